"""bench.py --dump-outputs and the plain / --full split.

CPU: dump_outputs writes float64, whole below the cap and the same seeded
sample above it.  GPU: one plain run on a small mesh -- the JSON line carries
the headline keys and none of the --full objects, --steps sets the timed
steps, and DIR/y.npy is bitwise the action of the same operator on the same
seeded global field (the scatter is deterministic)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

torch = pytest.importorskip("torch")


def test_dump_outputs_whole_and_sample(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    v = torch.arange(1000, dtype=torch.float64) * 0.5
    bench.dump_outputs(str(tmp_path / "a"), "y", v)
    a = np.load(tmp_path / "a" / "y.npy")
    assert a.dtype == np.float64 and np.array_equal(a, v.numpy())
    monkeypatch.setattr(bench, "DUMP_MAX_VALUES", 64)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), "y", v)
    b, c = np.load(tmp_path / "b" / "y.npy"), np.load(tmp_path / "c" / "y.npy")
    assert b.dtype == np.float64 and b.shape == (64,) and np.array_equal(b, c)
    assert np.all(np.diff(b) >= 0) and np.isin(b, a).all()  # entries of v at sorted indices
    # several ranks: one file per rank, the cap shared
    bench.dump_outputs(str(tmp_path / "d"), "y", v, rank=1, world=4)
    assert np.load(tmp_path / "d" / "y_rank1.npy").shape == (16,)


@pytest.mark.gpu
def test_plain_run_and_dump(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    cfg = ["--p", "4", "--nex", "13", "--ney", "9"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps",
                        "3", "--warmup", "1", "--dump-outputs", str(tmp_path)] + cfg,
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["steps"] == 3 and res["ms_per_step"] > 0 and res["unit"] == "DOF/s"
    assert res["higher_is_better"] is True and res["dtype"] == "f64"
    assert abs(res["value"] - res["config"]["ndof_global"] / (res["ms_per_step"] * 1e-3)) \
        <= 1e-9 * res["value"]
    assert "parity" not in res and "cpu_baseline" not in res
    assert res["config"]["kernel_ms_quartiles"] is None
    y = np.load(tmp_path / "y.npy")
    assert y.dtype == np.float64
    sys.path.insert(0, ROOT)
    from bench import global_random_field
    from spectralelementmethod_amd.distributed import OverlappedOperator, StripPartition
    dev = torch.device("cuda", 0)
    part = StripPartition(13, 9, 4, 1, 0)
    nodes, e2n = part.local_mesh(0.05)
    op = OverlappedOperator(4, nodes, e2n, {}, 1, dev, world=1, rank=0)
    ref = op.apply(global_random_field(part, 1, 0, op.ndof, dev)).cpu().numpy()
    op.close()
    assert y.shape == ref.shape and np.array_equal(y, ref)
