"""A plain `bench.py --gpus 1 --steps K --warmup W` run times the headline
only and, with --dump-outputs DIR, writes what its last timed step computed:
the root (ref, size, block size, Posts) and the ctext.  At 8 MiB (8 blocks of
1 MiB + the index node) the ctext fits the dump whole, so every byte of it
and the root are compared with the oracle's writer over the same stream."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIB = 1 << 20
EXTRA_LEGS = {"roofline", "valu", "cpu_baseline", "host_round_trip", "config2", "small_blobs",
              "small_blobs_from_host", "config4_end_to_end", "concat", "postblob_latency",
              "postblob_concurrency"}


def test_plain_run_dumps_the_last_steps_outputs(gpu, O, tmp_path):
    size, seed = 8 * MIB, 3
    out = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                        "--steps", "3", "--warmup", "1", "--size-gib", str(size / (1 << 30)),
                        "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    rec = json.loads(lines[0])
    assert (rec["steps"], rec["warmup"], rec["n_gpus"]) == (3, 1, 1)
    assert rec["ms_per_step"] > 0 and rec["unit"] == "GiB/s" and rec["higher_is_better"] is True
    # both figures come from the one wall time; ms_per_step is rounded to 1 us
    # (5 % covers that rounding down to a 10 us step)
    assert rec["value"] == pytest.approx(size / (1 << 30) / (rec["ms_per_step"] * 1e-3), rel=0.05)
    assert not EXTRA_LEGS & set(rec), EXTRA_LEGS & set(rec)
    assert rec["fused_reruns"] == {"headline": 0}

    want_root, wsize, wbs, posts = O.create(O.fill_splitmix(size, seed), MIB, salt=None)
    assert sorted(os.listdir(out)) == ["ctext_sample.npy", "root_ref.npy",
                                       "root_size_bs_posts.npy"]
    ref = np.load(out / "root_ref.npy")
    assert ref.dtype == np.float32
    assert bytes(ref.astype(np.uint8)) == want_root
    assert rec["root_cid"] == want_root[:32].hex()
    shape = np.load(out / "root_size_bs_posts.npy")
    assert shape.dtype == np.float64 and shape.tolist() == [wsize, wbs, len(posts)]
    ct = np.load(out / "ctext_sample.npy")
    assert ct.dtype == np.float32 and ct.size == size
    want_ct = b"".join(c for _, _, _, c in posts[:size // MIB])
    assert bytes(ct.astype(np.uint8)) == want_ct
