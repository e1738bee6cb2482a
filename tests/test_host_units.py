"""The units that need no GPU, as stand-alone programs built with the host
compiler under AddressSanitizer and UBSan (tests/cunit.py): the host runtime's
DevicePool and job builders (glfs_amd/csrc/host.h,
tests/c/host_units_test.cpp), and the launch layer's per-stream scratch,
launch plans and launch log (stream_scratch.h, launch_plan.h, launch_log.h;
tests/c/stream_scratch_test.cpp, over a fake HIP runtime of its own).  Each
runs as its own process: nothing is loaded into Python and no GPU call is
made."""
from cunit import build_and_run


def test_pool_and_job_builders_under_sanitizers(tmp_path):
    build_and_run(tmp_path, "host_units_test")


def test_stream_scratch_and_launch_plan_under_sanitizers(tmp_path):
    build_and_run(tmp_path, "stream_scratch_test")
