"""`bench.py --gpus 1 --steps K --warmup W` is lean - the headline line only, the extras sit behind `--full` - and
`--dump-outputs DIR` writes what the timed path computed in its last step: for the refine the seeded batch's
`pose_i` / `scale_i`, the same arrays a caller of `model.refine` gets; for `--mode train` the last iteration's outputs, its
loss terms and the parameters after the last optimizer step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRAS = {"roofline", "maxpool_standalone", "split_mode", "single_image", "train_fp32", "cpu_baseline"}


def _bench(*args):
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.pop("CATRE_BENCH_DRYRUN", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_refine_line_is_lean_and_dumps_the_last_timed_step(tmp_path):
    line = _bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path))
    assert line["metric"] == "pose-refine iters/sec (B=256, N=1024, K=4)" and line["unit"] == "object-iterations/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f32" and line["value"] > 0
    assert line["steps"] == 3 and abs(line["per_rank_ms"][0] - 3 * line["ms_per_step"]) < 0.01   # --steps is the timed count
    assert not EXTRAS & set(line), sorted(EXTRAS & set(line))

    from catre_amd import synth
    from catre_amd.CATRE_disR_shared import build_model_optimizer, expected_state_shapes
    from catre_amd.config import default_cfg

    cfg = default_cfg(num_pcl=1024, num_kps=1024, n_iter=4, device="cuda:0")
    model, _ = build_model_optimizer(cfg, is_test=True)
    sd = synth.recipe_state_dict(expected_state_shapes(cfg))
    model.load_state_dict({k: v.cuda() for k, v in sd.items()}, strict=True)
    batch = {k: v.cuda() for k, v in synth.make_inputs(256, 1024, 1024, seed=1000).items()}   # rank 0's seeded batch
    want = model.eval().refine(batch, n_iter=4)
    assert sorted(f[:-4] for f in os.listdir(tmp_path)) == sorted(want)
    for k, v in want.items():
        got = np.load(tmp_path / f"{k}.npy")
        assert got.dtype == np.float32 and got.shape == tuple(v.shape), k
        err = float(np.abs(got - v.cpu().numpy()).max())
        assert err <= 1e-5, f"{k}: {err:.3e}"


def test_plain_train_line_dumps_outputs_losses_and_parameters(tmp_path):
    line = _bench("--mode", "train", "--steps", "1", "--warmup", "1", "--dump-outputs", str(tmp_path))
    assert line["steps"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    from catre_amd.CATRE_disR_shared import build_model_optimizer
    from catre_amd.config import default_cfg

    model, _ = build_model_optimizer(default_cfg(num_pcl=1024, num_kps=1024, n_iter=4, device="cpu"), is_test=False)
    names = {f[:-4] for f in os.listdir(tmp_path)}
    assert {"pose_4", "scale_4"} <= names
    assert {n[len("param."):] for n in names if n.startswith("param.")} == {k for k, _ in model.named_parameters()}
    assert any(n.startswith("loss.") for n in names)
    total = 0
    for n in names:
        a = np.load(tmp_path / f"{n}.npy")
        assert a.dtype == np.float32 and np.isfinite(a).all(), n
        total += a.nbytes
    assert total <= 64 * 2**20
    assert np.load(tmp_path / "pose_4.npy").shape == (256, 3, 4)
