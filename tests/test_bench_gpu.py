"""bench.py's plain run on the GPU: ONE JSON line with the headline keys over exactly --steps timed steps, none of the
--full extras, and --dump-outputs writing what the last timed step computed (the disk-integrated albedo and the
per-angle xint_at_top, float64) -- checked against the CPU oracle on the same seeded scene."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TTHG = (1.0, -1.0, 2.0, -0.5, 1.0)


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(tmp_path, oracle):
    from picaso_amd import disco, resident
    from picaso_amd import synthetic as syn
    nwno, nlayer, ng = 20000, 90, 5
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--nwno", str(nwno), "--prewarm-ms", "20", "--dump-outputs", str(tmp_path / "out")],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["unit"] == "spectra/s" and out["higher_is_better"] is True and out["dtype"] == "f64"
    assert out["steps"] == 3 and out["ms_per_step"] > 0
    assert out["value"] * out["ms_per_step"] == pytest.approx(1e3)          # one spectrum per step
    assert out["repeats"] is None and out["cold_ms_first_20"] is None
    assert not set(out) & {"cpu_baseline", "steady_state", "throughput_batched", "secondary", "product", "per_rank"}

    alb = np.load(tmp_path / "out" / "albedo.npy")
    xint = np.load(tmp_path / "out" / "xint_at_top.npy")
    assert sorted(os.listdir(tmp_path / "out")) == ["albedo.npy", "xint_at_top.npy"]
    assert alb.dtype == np.float64 and alb.shape == (nwno,) and xint.dtype == np.float64 and xint.shape == (ng, 1, nwno)

    # bench.py's scene (seed 3) on the CPU oracle, first 256 columns
    ns = 256
    sc = syn.make_scene(nlayer, nwno, seed=3)
    g, gw, t, tw = disco.get_angles_1d(ng)
    u0, u1, _, _, _ = disco.compute_disco(ng, 1, g, t, 0.0)
    planes = [np.ascontiguousarray(sc[k][:, :ns]) for k in resident.REFLECTED_PLANES]
    xo, _ = oracle.get_reflected_1d(nlayer + 1, sc["wno"][:ns], ns, ng, 1, *planes, 0.0, u0, u1, 1.0, np.ones(ns), 3, 0,
                                    *TTHG)
    ao = oracle.compress_disco(ns, 1.0, xo, gw, tw, np.ones(ns))
    assert np.max(np.abs(xint[..., :ns] - xo) / np.abs(xo)) < 1e-8
    assert np.max(np.abs(alb[:ns] - ao) / np.abs(ao)) < 1e-8
