"""The module-level drop-in of INTEGRATION.md section 1, executed for real against a stand-in host checkout.

The test writes a minimal `tmglow/`-style host tree into a temporary directory: an `args.py` with a `Parser` (the host
configuration the drop-in leaves alone), the host-only modules `utils/viz.py` and `pc/grad1Filter.py`, and host copies of
every module this package provides, which raise when imported (so a shadowing failure cannot pass unnoticed).  A child
process puts `deep-turbulence_amd/` AHEAD of that tree on sys.path and then runs the call sequence of `main.py` that
INTEGRATION.md section 1 lists: the import block (:13-24), `Parser().parse()` (:31), `Log` (:35), the model construction
(:61-72), the wrapper / optimizer / scheduler (:76-79), the data loaders (:86), the trainer (:87) and a workspace save / load
(:120, :34).  Everything up to the first kernel launch runs on the CPU (`args.src_device = "cpu"`), so this checks that every
name `main.py` imports resolves, resolves to THIS package where it provides the module, and accepts the arguments main.py
passes."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "deep-turbulence_amd")

# the stand-in host checkout: relative path -> file content
HOST_ARGS = r'''
import argparse, os, torch


class Parser(argparse.ArgumentParser):
    """Host configuration: the options main.py reads, with the cylinder-array case defaults filled in by parse()."""
    def __init__(self):
        super().__init__(description="stand-in host parser")
        self.add_argument("--exp-dir", type=str, default="./experiments")
        self.add_argument("--exp-type", type=str, default="backward-step", choices=["backward-step", "cylinder-array"])
        self.add_argument("--enc-blocks", nargs="*", type=int, default=[4, 4, 4])
        self.add_argument("--glow-blocks", nargs="*", type=int, default=[16, 16, 16])
        self.add_argument("--growth-rate", type=int, default=4)
        self.add_argument("--init-features", type=int, default=16)
        self.add_argument("--rec-features", type=int, default=64)
        self.add_argument("--cond-features", type=int, default=32)
        self.add_argument("--drop-rate", type=float, default=0.0)
        self.add_argument("--bn-size", type=int, default=8)
        self.add_argument("--training_data_dir", type=str, default=None)
        self.add_argument("--testing_data_dir", type=str, default=None)
        self.add_argument("--ntrain", type=int, default=None)
        self.add_argument("--ntest", type=int, default=None)
        self.add_argument("--noise-std", type=float, default=None)
        self.add_argument("--max-grad-norm", type=float, default=None)
        self.add_argument("--noc", type=int, default=3)
        self.add_argument("--nic", type=int, default=None)
        self.add_argument("--glow_upscale", type=int, default=None)
        self.add_argument("--epoch_start", type=int, default=0)
        self.add_argument("--epochs", type=int, default=400)
        self.add_argument("--lr", type=float, default=0.001)
        self.add_argument("--beta", type=float, default=None)
        self.add_argument("--dx", type=float, default=None)
        self.add_argument("--dy", type=float, default=None)
        self.add_argument("--batch-size", type=int, default=None)
        self.add_argument("--test-batch-size", type=int, default=None)
        self.add_argument("--seed", type=int, default=12345)

    def parse(self):
        args = self.parse_args()
        case = dict(ntrain=96, ntest=4, noise_std=0.05, beta=200.0, dx=5.0 / 64, dy=5.0 / 64, batch_size=64, test_batch_size=4,
                    max_grad_norm=1.0, nic=3, glow_upscale=4)
        for k, v in case.items():
            if getattr(args, k) is None:
                setattr(args, k, v)
        args.run_dir = os.path.join(args.exp_dir, args.exp_type, "run")
        args.ckpt_dir = os.path.join(args.run_dir, "checkpoints")
        args.pred_dir = os.path.join(args.run_dir, "predictions")
        for d in (args.run_dir, args.ckpt_dir, args.pred_dir):
            os.makedirs(d, exist_ok=True)
        torch.manual_seed(args.seed)
        return args
'''
SHADOWED = "raise ImportError('host copy of %s imported: the drop-in package must shadow it')\n"
HOST = {
    "args.py": HOST_ARGS,
    "nn/__init__.py": "",
    "utils/__init__.py": "",
    "utils/viz.py": "HOST_ONLY = True\n",
    "pc/__init__.py": "",
    "pc/grad1Filter.py": "HOST_ONLY = True\n",
}
for _m in ("nn/tmGlow.py", "nn/trainFlowParallel.py", "utils/dataLoader.py", "utils/utils.py", "utils/log.py", "utils/parallel.py"):
    HOST[_m] = SHADOWED % _m

CHILD = r'''
import os, sys
PKG, REF, DATA = sys.argv[1:4]
sys.argv = ["main.py", "--exp-type", "cylinder-array", "--ntrain", "2", "--ntest", "1", "--batch-size", "2", "--test-batch-size", "1",
            "--training_data_dir", DATA, "--testing_data_dir", DATA, "--enc-blocks", "1", "1", "--glow-blocks", "2", "2",
            "--rec-features", "4", "--cond-features", "4", "--init-features", "8", "--exp-dir", os.path.join(DATA, "exp")]
sys.path[:0] = [PKG, REF]                       # INTEGRATION.md section 1: this package ahead of tmglow/
# main.py:13-24, the import block
from args import Parser
from nn.tmGlow import TMGlow
from nn.trainFlowParallel import TrainFlow
from utils.dataLoader import DataLoaderAuto
from utils.utils import saveWorkspace, loadWorkspace
from utils.log import Log
from utils.parallel import DataParallelINNModel
from torch.optim.lr_scheduler import ExponentialLR
import torch
import inspect
for obj, mod in ((TMGlow, "nn/tmGlow.py"), (TrainFlow, "nn/trainFlowParallel.py"), (DataLoaderAuto, "utils/dataLoader.py"),
                 (saveWorkspace, "utils/utils.py"), (Log, "utils/log.py"), (DataParallelINNModel, "utils/parallel.py")):
    f = inspect.getsourcefile(obj)
    assert f == os.path.join(PKG, mod), (obj.__name__, f)
assert inspect.getsourcefile(Parser) == os.path.join(REF, "args.py")   # host config stays the host's
import utils.viz, pc.grad1Filter                  # modules only the host has keep resolving (pkgutil.extend_path)
assert utils.viz.__file__.startswith(REF) and pc.grad1Filter.__file__.startswith(REF)
args = Parser().parse()                          # main.py:31
log = Log(args, record=True)                     # main.py:35
args.device, args.device_ids, args.src_device, args.n_gpu = torch.device("cpu"), [0], "cpu", 1
model = TMGlow(in_features=args.nic, out_features=args.noc, enc_blocks=args.enc_blocks, glow_blocks=args.glow_blocks,
               cond_features=args.cond_features, cglow_upscale=args.glow_upscale, growth_rate=args.growth_rate,
               init_features=args.init_features, rec_features=args.rec_features, bn_size=args.bn_size, drop_rate=args.drop_rate,
               bottleneck=False).to(args.src_device)                                      # main.py:61-72
model = DataParallelINNModel(model, args.device_ids)                                      # main.py:76-79
optimizer = torch.optim.Adam(model.parameters(), lr=args.lr * (0.995 ** args.epoch_start), weight_decay=1e-8, amsgrad=True)
scheduler = ExponentialLR(optimizer, gamma=0.995)
data_loader, training_loader, testing_loader = DataLoaderAuto.init_data_loaders(args, model, log)    # main.py:86
trainer = TrainFlow(args, model, training_loader, testing_loader, log=log)                            # main.py:87
assert type(model).__name__ == "DataParallelINNModel" and type(model.module).__name__ == "TMGlow"
x, y, seeds = next(iter(training_loader))
assert x.shape[0] == 2 and x.shape[2] == 3 and y.shape[-1] == 4 * x.shape[-1] and seeds.shape == (2,)
assert float(model.module.out_std.abs().sum()) > 0          # transferNormalizingParams reached the wrapped model
assert hasattr(trainer, "trainParallel") and hasattr(trainer, "test")
saveWorkspace(args, model.module, optimizer, file_id=1)     # main.py:120
assert loadWorkspace(args, args.ckpt_dir, file_id=1) is not None   # main.py:34
print("SWAP-OK", len(list(model.parameters())))
'''


def test_main_py_import_block_and_construction_resolve_here(tmp_path):
    rs = np.random.RandomState(5)
    for case in (0, 95, 96):
        np.savez(os.path.join(tmp_path, "cylinderArrayCoarse%d-[U,p].npz" % case), data=rs.standard_normal((4, 4, 4, 4)).astype(np.float32))
        np.savez(os.path.join(tmp_path, "cylinderArrayFine%d-[U,p].npz" % case), data=rs.standard_normal((4, 4, 16, 16)).astype(np.float32))
    ref = tmp_path / "host" / "tmglow"
    for rel, text in HOST.items():
        (ref / rel).parent.mkdir(parents=True, exist_ok=True)
        (ref / rel).write_text(text)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="", MPLBACKEND="Agg", PYTHONDONTWRITEBYTECODE="1")
    env.pop("PYTHONPATH", None)
    r = subprocess.run([sys.executable, "-c", CHILD, PKG, str(ref), str(tmp_path)], cwd=str(tmp_path), env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "SWAP-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
