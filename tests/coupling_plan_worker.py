"""Worker of tests/test_coupling_kernels.py::test_launch_plans_in_a_fresh_process: runs a handful of the fp64-checked coupling and
growth-layer backward cases in a process of its own, started with TMG_CPL_GRID=5 TMG_D2_BLOCKS=3 (the launchers read both once per
process).  Exit status 0 and the closing line mean every case held its bounds."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import common as C  # noqa: E402,F401  (sets sys.path)
import test_coupling_kernels as T  # noqa: E402


if __name__ == "__main__":
    T.run_forced_plan_cases()
    print("forced launch plans: ok")
