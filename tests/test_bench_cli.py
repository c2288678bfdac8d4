"""bench.py's command line: a plain run does only the headline (no `--full` fields), `--steps` sets the timed steps,
`ms_per_step` is their time, and `--dump-outputs DIR` writes the last timed step's outputs - computed from the same inputs on
every run, so two runs agree to the rounding of one step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import common as C

FULL_ONLY = ("roofline", "cpu_baseline", "cpu_baseline_cfg1", "density_direction", "wino_bf16x3_variant", "mix_f16_variant",
             "mix_f16_speedup", "hbm_kernel_classes", "mix_1x1_mfma")


def test_dump_outputs_is_bounded_and_seeded(tmp_path):
    import bench
    from nn.tmGlow import TMGlow
    model = TMGlow(**C.build_kwargs(C.CFG_TINY))
    for p in model.parameters():
        p.grad = torch.full_like(p, 0.5)
    nparam = sum(p.numel() for p in model.parameters())
    big = torch.arange(3 * bench.DUMP_CAP_DEFAULT, dtype=torch.float64)
    outs = {"y": big, "logdet": torch.ones(5), "states": [(torch.zeros(2, 3), torch.ones(4)), (torch.ones(1), torch.zeros(1))],
            "loss": torch.tensor(2.0)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), outs, model)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["grads.npy", "logdet.npy", "loss.npy", "states.npy", "y.npy"]
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == np.float32 and a.ndim == 1
        np.testing.assert_array_equal(a, b)                       # the same sample on every run
        total += a.nbytes
    assert total <= bench.DUMP_MAX_BYTES
    y = np.load(tmp_path / "a" / "y.npy")
    assert y.size == bench.DUMP_CAP_DEFAULT and (np.diff(y) >= 0).all() and y.max() < big.numel()   # sorted sample of the entries
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "states.npy"), [0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 0])
    assert np.load(tmp_path / "a" / "loss.npy").tolist() == [2.0]
    assert np.load(tmp_path / "a" / "grads.npy").size == nparam and (np.load(tmp_path / "a" / "grads.npy") == 0.5).all()


def test_restart_from_gives_the_step_of_a_fresh_optimizer():
    """The last timed step of a --dump-outputs run starts from the seeded state: after restart_from, a step equals the first step
    of a fresh model and optimizer, bit for bit, whatever steps came before."""
    import bench
    from nn.tmGlow import TMGlow

    def make():
        C.seed_all(3)
        m = TMGlow(**C.build_kwargs(C.CFG_TINY))
        return m, torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-8, amsgrad=True)

    def step(m, opt, seed):
        g = torch.Generator().manual_seed(seed)
        opt.zero_grad(set_to_none=True)
        for p in m.parameters():
            p.grad = torch.randn(p.shape, generator=g)
        opt.step()

    m, opt = make()
    start = {k: v.detach().clone() for k, v in m.state_dict().items()}
    for s in range(3):
        step(m, opt, 10 + s)
    bench.restart_from(m, opt, start)
    step(m, opt, 99)
    ref, ref_opt = make()
    step(ref, ref_opt, 99)
    for (k, a), b in zip(m.state_dict().items(), ref.state_dict().values()):
        assert torch.equal(a, b), k
    for p, q in zip(m.parameters(), ref.parameters()):
        for key, v in ref_opt.state[q].items():
            assert torch.equal(opt.state[p][key], v), key


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    runs = []
    for d in ("a", "b"):
        cmd = [sys.executable, os.path.join(C.ROOT, "bench.py"), "--gpus", "1", "--config", "tiny", "--steps", "3", "--warmup", "2",
               "--dump-outputs", str(tmp_path / d)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, lines
        runs.append(json.loads(lines[0]))
    for out in runs:
        assert out["steps"] == 3 and out["warmup"] == 2 and out["ms_per_step"] > 0 and out["higher_is_better"] is True
        assert abs(out["value"] - 2 * 3 / (out["ms_per_step"] * 3e-3)) < 1e-2 * out["value"]
        assert out["dtype"] == "f32" and out["unit"] == "samples/s"
        assert not [k for k in FULL_ONLY if out.get(k) is not None], out
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["grads.npy", "logdet.npy", "loss.npy", "states.npy", "y.npy"]
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == np.float32 and a.shape == b.shape and np.isfinite(a).all()
        # same inputs, same latents: the runs differ only by the order of float atomics within the one dumped step
        assert np.abs(a - b).max() <= 1e-4 * (np.abs(b).max() + 1e-6), n
    assert np.load(tmp_path / "a" / "loss.npy")[0] == pytest.approx(runs[0]["config"]["loss_last"], rel=1e-6)
