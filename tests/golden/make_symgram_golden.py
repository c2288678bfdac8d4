"""Writes the fixtures that pin the shared symmetric-Gram engine (csrc/tmg_symgram.h) and the shared slice rounding to the commit before
them, from the library that is built in the tree.  Run it at THAT commit (with these tests' files beside it), never to make a failing
test pass:
  python tests/golden/make_symgram_golden.py --plans    tests/golden/symgram_plans.json: the raw output of the four plan entries over
                                                        the grid of tests/test_symgram_cpu.py (host code, no device)
  python tests/golden/make_symgram_golden.py --bits     tests/golden/symgram_bits.json: SHA-256 of the outputs of the real-data cases
                                                        of tests/test_energy_gpu.py and tests/test_spod_gpu.py (on an MI355X)
--out DIR writes the file into another directory."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plans", action="store_true")
    ap.add_argument("--bits", action="store_true")
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.plans:
        import test_symgram_cpu as T
        rec = {e: [[d, T.evaluate(e, d)] for d in T.grid(e)] for e in sorted(T.OUT)}
        json.dump(rec, open(os.path.join(a.out, "symgram_plans.json"), "w"), separators=(",", ":"))
    if a.bits:
        import test_energy_gpu as E
        import test_spod_gpu as S
        rec = {"gram": {}, "spod": {}}
        for row in E.BITS_ROWS:
            sha, plan = E.energy_bits(*row)
            rec["gram"][E.bits_name(row)] = {"plan": plan, "sha256": sha}
        for c in S.BITS_CASES:
            sha, plan = S.csd_bits(*c)
            rec["spod"][S.bits_name(c)] = {"plan": plan, "sha256": sha}
        json.dump(rec, open(os.path.join(a.out, "symgram_bits.json"), "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
