"""bench.py --dump-outputs on the GPU: the dump is the timed path's state after exactly --warmup + --steps ticks (checked against the
oracle stepped as many ticks), and two runs of the same command line dump the same outputs."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O
from tests.util import compare_constraints, oracle_world, rel_err

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_dump(out, steps, warmup):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--tile", "8", "8", "8", "--steps", str(steps), "--warmup", str(warmup),
           "--min-seconds", "0", "--no-settled", "--no-other-configs", "--no-order-check", "--no-cpu-baseline", "--dump-outputs", str(out)]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return {f[:-4]: np.load(os.path.join(out, f)) for f in os.listdir(out) if f.endswith(".npy")}


def test_dump_is_the_state_after_warmup_plus_steps_ticks(tmp_path):
    from mgf_amd import scenes
    steps, warmup = 3, 2
    got = _bench_dump(tmp_path / "a", steps, warmup)
    scene = scenes.sphere_pile(8, 8, 8)
    dt, iters = float(scene["dt"]), scene["iters"]
    ow = oracle_world(scene, O.ORDER_CANONICAL)
    for _ in range(warmup + steps):
        st = ow.step(dt, iters)
    want = ow.state()
    assert np.array_equal(got["body_rows"], np.arange(512))
    for k in ("x", "q", "v", "omega", "delta"):
        assert got[k].dtype == np.float32 and rel_err(got[k], want[k]) <= 1e-4, k
    cons = ow.constraints()
    assert got["step_stats"][0] == 512 and got["step_stats"][1] == st.n_constraints == len(cons) == len(got["constraint_rows"])
    dumped = np.zeros(len(cons), cons.dtype)
    for f in cons.dtype.names:
        dumped[f] = got["constraint_" + f]
    compare_constraints(dumped, cons)
    again = _bench_dump(tmp_path / "b", steps, warmup)
    assert got.keys() == again.keys() and all(np.array_equal(got[k], again[k]) for k in got)
