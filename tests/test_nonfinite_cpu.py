"""nonfinite_cases.py without a device ("Non-finite values"): the fp64 references do what the contract assumes, the Winograd
footprint is capped, and the judge is sharp.

  test_reference_has_the_expected_nonfinite_set   per case and poison: the reference R is non-finite exactly where the geometry says
        (a 3x3 convolution: the neighbourhood that reads the pixel, all output channels; a weight gradient: the poisoned channel's
        column; pointwise: the element; train-mode BatchNorm: the channel), finite elsewhere, and not vacuous; -Inf behind a ReLU and
        +-Inf behind a clamp leave R finite
  test_wino_footprint_is_capped                   at most 16 output pixels per poisoned pixel on every Winograd case, every pixel
  test_the_judge_passes_the_reference_itself      R judged against R: nothing swallowed, leaked or off
  test_mutated_reference_is_caught                a reference mutated the way the kernels behaved (relu(NaN) = 0, clamp(NaN) = lower limit,
        vmax kept, std = 0 at a NaN second moment) trips rule 1 on every case that has such a site
  test_all_nan_reference_leaks                    a reference turned NaN everywhere trips rule 2
  test_every_family_is_named, test_adam_formula_and_torch_optim_agree_on_the_nonfinite_set"""
import math

import pytest
import torch

import common as C  # noqa: F401  (sets sys.path)
import nonfinite_cases as N
import wino_cases as WC

FAMILIES = {"conv_fwd": "conv_fwd", "conv_wgrad": "conv_wgrad", "conv_dgrad": "conv_dgrad_direct", "conv_border": "conv_rep_border_fix",
            "wino_fwd": "conv_wino_fwd", "wino_narrow": "conv_wino_narrow", "wino_wgrad": "conv_wino_wgrad",
            "wino_wgrad_grouped": "conv_wgrad_grouped", "gauss": "gauss_fwd", "gauss_sample": "gauss_sample", "adam": "adam_step",
            "batchnorm": "bn_finalize64", "ensemble": "ens_accum", "phys_fwd": "phys_fwd", "phys_rms": "phys_rms", "phys_fields": "phys_fields",
            "phys_bwd": "phys_bwd", "thin": "c1_fwd",
            "coupling_fwd": "coupling_fwd", "coupling_bwd": "coupling_bwd", "dense2_bwd": "dense2_bwd", "masked_add": "masked_add",
            "affine_apply": "affine_apply", "affine_bwd": "affine_bwd", "thin_wgrad": "conv_wgrad_thin_grouped", "c1_bwd": "c1_bwd", "node": "CouplingTailFn", "model": "TMGlow.reconstruct"}
NODE_ENTRIES = {"CouplingTailFn", "ConvLSTMCellFn", "DenseBlockFn", "MixFn", "ConvFn"}


def _H():
    import tmg_hip as H
    H.lib()          # the planners name the batch of the plan-dependent cases; they need the library, not a device
    return H


def _params(pred=lambda c, lab: True):
    return [pytest.param(c, lab, id="%s-%s-%s" % (c["family"], c["name"], lab)) for c in N.CASES for lab in c["labels"] if pred(c, lab)]


@pytest.mark.parametrize("case,label", _params())
def test_reference_has_the_expected_nonfinite_set(case, label):
    run = case["build"](label, _H())
    N.assert_not_vacuous(dict(run, glob=run["glob"] or label in case["glob"]))
    for name, R in run["R"].items():
        e = run["expect"].get(name)
        nf = N.nonfinite(R)
        if run["finite"]:
            assert not bool(nf.any()), name
        elif e is not None and run["exact"]:
            assert torch.equal(nf, e.expand_as(nf).contiguous()), "%s: %d non-finite, %d expected" % (name, int(nf.sum()), int(e.sum()))
        elif e is not None:
            assert not bool((nf & ~e.expand_as(nf)).any()), "%s: non-finite outside the reach of the poisoned element" % name
        assert bool(torch.isfinite(run["bound"][name] if torch.is_tensor(run["bound"][name]) else torch.tensor(0.0)).all()), name
    # pointwise kernels: one element; BatchNorm in train mode: the whole channel
    if case["family"] == "adam":
        assert all(int(N.nonfinite(R).sum()) == 1 for n, R in run["R"].items() if n != "vm" or run["d"]["ams"])
    if case["family"] == "gauss" and not run["finite"]:
        assert int(N.nonfinite(run["R"]["logp"]).sum()) <= 1          # one image; mode 1's log-probability does not read the mean
        assert all(int(N.nonfinite(run["R"][n]).sum()) <= 2 for n in ("zout", "dzout", "dhz") if n in run["R"])
    if case["family"] == "batchnorm":
        for n in ("mean", "var", "rstd", "a", "bsh", "running_mean", "running_var") if label.startswith("x.") else ("a", "bsh"):
            assert int(N.nonfinite(run["R"][n]).sum()) == 1, n
        nfx = N.nonfinite(run["R"]["dx"])
        assert bool(nfx.flatten(0, 2).all(0).sum() == 1) and int(nfx.sum()) == nfx[..., 0].numel()


@pytest.mark.parametrize("case", [c for c in N.CASES if c["family"] in ("wino_fwd", "wino_narrow")], ids=lambda c: c["name"])
def test_wino_footprint_is_capped(case):
    name = case["name"].rsplit("-", 1)[0] if case["family"] == "wino_fwd" else case["name"]
    wc = (WC.NARROW_BY_NAME if case["family"] == "wino_narrow" else WC.FWD_BY_NAME)[name]
    Hh, Ww = wc["hw"]
    for rep in (False, True):
        for y in range(Hh):
            for x in range(Ww):
                m = N.wino_footprint((2, Hh, Ww), (1, y, x), rep)
                assert 1 <= int(m.sum()) <= N.WINO_FOOTPRINT_CAP and not bool(m[0].any()), (y, x, rep)
                # the footprint holds every output that reads the pixel: the exception never hides a swallowed element
                assert not bool((N.conv_reach((2, Hh, Ww), (1, y, x), 3, 1, rep) & ~m).any()), (y, x, rep)
    # and the cases' own runs stay inside it
    for label in case["labels"]:
        run = case["build"](label, _H())
        a = run.get("allowed", {}).get("out")
        if a is not None:
            assert int(a[..., 0].sum()) <= N.WINO_FOOTPRINT_CAP and not bool((N.nonfinite(run["R"]["out"]) & ~a).any()), label


@pytest.mark.parametrize("case,label", _params(lambda c, lab: lab.endswith(".nan")))
def test_the_judge_passes_the_reference_itself(case, label):
    run = case["build"](label, _H())
    assert not N.failures(N.judge(run, run["R"]))


@pytest.mark.parametrize("case,label", _params(lambda c, lab: bool(c["sites"]) and lab.endswith(".nan")))
def test_mutated_reference_is_caught(case, label):
    run = case["build"](label, _H())
    if not run["trips"]:
        return            # this poison passes no swallowing site of the case (a NaN weight, a mean that is not clipped)
    v = N.judge(run, {**run["R"], **run["mutated"]()})
    assert sum(r["swallowed"] for r in v.values()) > 0, (case["name"], label)


@pytest.mark.parametrize("case", [c for c in N.CASES if c["family"] == "batchnorm"], ids=lambda c: c["name"])
def test_dropped_mask_gradient_is_caught_by_rule_2(case):
    """The BatchNorm chain's mask site shows under rule 2: a reference whose mask drops the gradient at a NaN pre-activation leaves the
    poisoned channel's dbeta finite but off its bound."""
    run = case["build"]("x.a.nan", _H())
    assert bool(torch.isfinite(run["R"]["dbeta"]).all())
    v = N.judge(run, run["mutated"]())
    assert v["dbeta"]["off"] == 1 and v["dbeta"]["swallowed"] == 0


def test_every_case_with_a_site_has_a_poison_that_trips_it():
    H = _H()
    for case in N.CASES:
        if case["sites"] and "mask" not in case["sites"]:       # the mask sites show under rule 2 (finite references)
            assert any(case["build"](lab, H)["trips"] for lab in case["labels"] if lab.endswith(".nan")), case["name"]


@pytest.mark.parametrize("case", [c for c in N.CASES if c["family"] != "model"], ids=lambda c: "%s-%s" % (c["family"], c["name"]))
def test_all_nan_reference_leaks(case):
    label = [lab for lab in case["labels"] if lab.endswith(".nan")][0]
    run = case["build"](label, _H())
    if all(bool(N.nonfinite(R).all()) for R in run["R"].values()):
        return            # a global operation: there is no finite element to leak into
    v = N.judge(run, {n: torch.full_like(R, float("nan")) for n, R in run["R"].items()})
    assert sum(r["leaked"] for r in v.values()) > 0 and sum(r["swallowed"] for r in v.values()) == 0


def test_verdict_counts():
    R = torch.tensor([1.0, float("nan"), float("inf"), 2.0, 3.0])
    A = torch.tensor([1.0, 0.0, float("nan"), float("nan"), 3.5])
    v = N.verdict(A, R, 0.25)
    assert (v["swallowed"], v["leaked"], v["off"]) == (1, 1, 1)
    free = torch.tensor([False, False, False, True, True])
    v = N.verdict(A, R, 0.25, free)
    assert (v["swallowed"], v["leaked"], v["off"]) == (1, 0, 0)


def test_every_family_is_named():
    have = {c["family"] for c in N.CASES}
    assert have == set(FAMILIES), have ^ set(FAMILIES)
    for fam, entry in FAMILIES.items():
        assert any(entry in c["entry"] for c in N.CASES if c["family"] == fam), fam
    assert any("c1x2_fwd" in c["entry"] for c in N.CASES)
    assert {c["entry"][0] for c in N.CASES if c["family"] == "node"} == NODE_ENTRIES
    assert {"dense-d6-train", "dense-d6-eval"} <= {c["name"] for c in N.CASES if c["family"] == "node"}
    assert {c["name"].rsplit("-", 1)[1] for c in N.CASES if c["family"] == "wino_fwd"} == {"f32", "bf16x3"}
    assert set(N.POISONS) == {"nan", "pinf", "ninf"} and math.isnan(N.POISONS["nan"])


def test_adam_formula_and_torch_optim_agree_on_the_nonfinite_set():
    """test_param_kernels.adam_ref is the reference the kernel is judged by; torch.optim.Adam in fp64 on the same poisoned gradient is
    non-finite in the same elements of p, m, v and vmax."""
    import test_param_kernels as PK
    for name, (wd, ams, step) in N.ADAM.items():
        for label in ("g.a.nan", "g.b.nan", "g.a.pinf", "g.b.ninf"):
            run = N.build_adam(name, label, None)
            vals = run["d"]["vals"]
            p = torch.nn.Parameter(vals["p"].double().clone())
            opt = torch.optim.Adam([p], lr=PK.LR, betas=(PK.B1, PK.B2), eps=PK.AEPS, weight_decay=wd, amsgrad=bool(ams))
            st = opt.state[p]
            st["step"] = torch.tensor(float(step - 1))
            st["exp_avg"], st["exp_avg_sq"] = vals["m"].double().clone(), vals["v"].double().clone()
            if ams:
                st["max_exp_avg_sq"] = vals["vm"].double().clone()
            p.grad = vals["g"].double().clone()
            opt.step()
            got = {"p": p.detach(), "m": st["exp_avg"], "v": st["exp_avg_sq"]}
            if ams:
                got["vm"] = st["max_exp_avg_sq"]
            for k, t in got.items():
                assert torch.equal(N.nonfinite(t), N.nonfinite(run["R"][k])), (name, label, k)
                fin = torch.isfinite(t)
                assert bool(((t - run["R"][k])[fin].abs() <= 1e-6 * (1 + run["R"][k][fin].abs())).all()), (name, label, k)
