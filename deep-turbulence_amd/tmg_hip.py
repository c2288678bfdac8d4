"""ctypes binding of libtmglow_hip.so (C ABI: include/tmglow_hip.h) for PyTorch-ROCm tensors.

PyTorch is plumbing here: device memory (caching allocator), the current HIP stream and autograd
bookkeeping.  Every numerical operation of the hot path is a kernel of the shared library.  There is
no CPU or eager fallback: calling an op without the library, or with a tensor that is not a
contiguous-NHWC fp32 CUDA/HIP tensor, raises.

Internal tensor convention: activations are torch tensors of shape [B, H, W, C] (NHWC, contiguous)
or channel-slice views of such tensors.  `seg(t)` turns one into the (pointer, stride, offset, n)
descriptor the library expects.
"""
import ctypes
import os
import weakref
import subprocess
import sys

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libtmglow_hip.so")
CSRC = os.path.join(_HERE, "csrc")
SOURCES = ["tmg_conv.hip", "tmg_pointwise.hip", "tmg_physics.hip", "tmg_mix16.hip", "tmg_coupling.hip", "tmg_wino.hip", "tmg_thin.hip", "tmg_glue.hip", "tmg_ensemble.hip", "tmg_spectrum.hip", "tmg_scores.hip", "tmg_tspec.hip", "tmg_quant.hip", "tmg_gram.hip", "tmg_sfun.hip", "tmg_event.hip", "tmg_pdf.hip", "tmg_pod.hip", "tmg_phase.hip", "tmg_spod.hip", "tmg_budget.hip", "tmg_corr.hip", "tmg_flux.hip", "tmg_vortex.hip", "tmg_frank.hip", "tmg_xspec.hip", "tmg_spell.hip", "tmg_iscale.hip", "tmg_mink.hip", "tmg_edt.hip", "tmg_lspec.hip", "tmg_lagr.hip"]
# Sources compiled WITHOUT the packed-fp32 vector instructions (v_pk_add_f32 / v_pk_fma_f32 / v_pk_mul_f32): beside MFMAs a packed
# f32 instruction costs ~13 cycles more than the two scalar ones it replaces (MI355X_MICROARCH.md, cycle constants, 'price of one
# filler beside MFMAs'), and the compiler SLP-packs adjacent scalar adds / multiplies by itself under -O3.  The matrix-core kernels'
# files are listed; the vector-ALU kernels (tmg_pointwise.hip, tmg_physics.hip) keep the packed forms, which double their arithmetic
# rate.  Round 3 measured the switch inside the noise and left the list empty; round 5 on one box, alternating three times: packed
# everywhere 43.62 / 43.98 / 43.76 ms per step, this list 43.51 / 43.60 / 43.37 (wino + conv + coupling alone 43.64 / 43.52 / 43.58).
# tmg_pod.hip is listed: its vector work (the fluctuation's subtraction and product, the energy's fmaf chain) is issued between the
# MFMAs of the projection, exactly the filler position the list is about; its results do not depend on the choice (a packed
# instruction rounds each half as the scalar one does).  tmg_spod.hip is listed for the same reason: the correction
# x - xbar G of every fragment element is vector work between the MFMAs of the Gram product and of the synthesis.
# tmg_xspec.hip is listed as tmg_spectrum.hip is: its column pass stores the accumulators between the MFMAs of the next row tile.
# tmg_lspec.hip likewise: the Welford updates of a mode tile's epilogue are vector work between the MFMAs of the next tile.
NO_PACKED_F32 = ["tmg_wino.hip", "tmg_conv.hip", "tmg_coupling.hip", "tmg_thin.hip", "tmg_mix16.hip", "tmg_spectrum.hip", "tmg_tspec.hip",
                 "tmg_pod.hip", "tmg_spod.hip", "tmg_xspec.hip", "tmg_lspec.hip"]
_lib = None

c_i64 = ctypes.c_int64
c_vp = ctypes.c_void_p

EXPORTS = [
    "tmg_conv_pack", "tmg_conv_pack_map", "tmg_conv_fwd", "tmg_conv_fwd_add", "tmg_affine_bwd_scaled", "tmg_c1_fwd_add", "tmg_conv_wgrad", "tmg_conv_wgrad_ws_floats", "tmg_conv_rep_border_fix", "tmg_conv_dgrad_direct",
    "tmg_affine_apply", "tmg_affine_apply_pass", "tmg_bn_finalize", "tmg_affine_bwd", "tmg_lstm_pointwise_fwd", "tmg_lstm_pointwise_bwd", "tmg_gauss_fwd",
    "tmg_gauss_bwd", "tmg_checker", "tmg_upsample_fwd", "tmg_upsample_bwd", "tmg_chan_reduce", "tmg_bn_bwd_apply",
    "tmg_phys_fwd", "tmg_phys_rms", "tmg_phys_bwd", "tmg_conv_wgrad_grouped", "tmg_conv_wgrad_grouped_ws_floats", "tmg_conv_pack_batched", "tmg_masked_add", "tmg_c1x2_fwd", "tmg_c1_fwd", "tmg_c1_bwd", "tmg_dense2_bwd", "tmg_dkappa", "tmg_prof_enable", "tmg_prof_collect", "tmg_mix_f16", "tmg_phys_bwd_dev", "tmg_coupling_fwd", "tmg_coupling_bwd",
    "tmg_conv_wino_pack", "tmg_conv_wino_fwd", "tmg_conv_wino_narrow", "tmg_conv_wino_wgrad", "tmg_conv_wino_wgrad_ws_floats", "tmg_mix_f32", "tmg_lu_fold_fwd", "tmg_lu_fold_bwd", "tmg_lu_fold_bwd_split", "tmg_level_finish", "tmg_conv_wgrad_thin_grouped", "tmg_mix_wgrad_grouped", "tmg_layer_planes", "tmg_conv_wino_wgrad_grouped", "tmg_conv_wino_wgrad_grouped_ws_floats", "tmg_adam_step", "tmg_chan_moments", "tmg_bn_finalize64", "tmg_mix_f32_affine_fwd", "tmg_mix_f32_affine_bwd", "tmg_conv_pack_many", "tmg_pad_halves", "tmg_coupling_fwd_halves", "tmg_coupling_bwd_halves", "tmg_fill_i64", "tmg_conv_wino_pack3", "tmg_conv_wino_fwd3", "tmg_mat_inverse", "tmg_gauss_sample", "tmg_reverse_loss_fwd", "tmg_reverse_loss_bwd", "tmg_sum_terms", "tmg_vec_sum", "tmg_level_pack", "tmg_spread2", "tmg_phys_fields", "tmg_phys_fields_bwd",
    "tmg_gauss_sample_keyed", "tmg_ens_accum", "tmg_ens_time_finalize", "tmg_ens_turb_accum", "tmg_ens_turb_finalize",
    "tmg_spec_rows", "tmg_spec_cols", "tmg_spec_accum", "tmg_spec_finalize",
    "tmg_ens_score_store", "tmg_ens_score_step",
]
# Launch-plan queries of the convolution launchers, direct (conv_fwd_plan / conv_wgrad_plan / conv_rep_border_plan below) and Winograd
# (conv_wino_fwd_plan / conv_wino_fwd3_plan / conv_wino_narrow_plan / conv_wino_wgrad_plan), and of the growth-layer forwards and the thin /
# mix weight gradients (c1x2_fwd_plan / c1_fwd_plan / conv_wgrad_thin_grouped_plan / mix_wgrad_grouped_plan): they launch nothing, so
# they are listed apart from the operations above.
PLAN_EXPORTS = ["tmg_conv_fwd_plan", "tmg_conv_wgrad_plan", "tmg_conv_rep_border_plan", "tmg_conv_wino_fwd_plan", "tmg_conv_wino_fwd3_plan",
                "tmg_conv_wino_narrow_plan", "tmg_conv_wino_wgrad_plan", "tmg_c1x2_fwd_plan", "tmg_c1_fwd_plan",
                "tmg_conv_wgrad_thin_grouped_plan", "tmg_mix_wgrad_grouped_plan"]
# The temporal power spectra (csrc/tmg_tspec.hip), declared in include/tmglow_hip_tspec.h: tspec_store / tspec_block / tspec_finalize below.
TSPEC_EXPORTS = ["tmg_tspec_store", "tmg_tspec_block", "tmg_tspec_finalize"]
# The prediction intervals (csrc/tmg_quant.hip), declared in include/tmglow_hip_quant.h: ens_quant_step below.
QUANT_EXPORTS = ["tmg_ens_quant_step"]
# The energy score and member distances (csrc/tmg_gram.hip), declared in include/tmglow_hip_gram.h: ens_gram_plan / ens_gram_step /
# ens_gram_traj below.
GRAM_EXPORTS = ["tmg_ens_gram_plan", "tmg_ens_gram_step", "tmg_ens_gram_traj"]
# The structure functions and the variogram score (csrc/tmg_sfun.hip), declared in include/tmglow_hip_sfun.h: ens_sfun_plan /
# ens_sfun_step below.
SFUN_EXPORTS = ["tmg_ens_sfun_plan", "tmg_ens_sfun_step"]
# The event verification: Brier, reliability, ROC, fractions skill score (csrc/tmg_event.hip), declared in
# include/tmglow_hip_event.h: ens_event_plan / ens_event_count / ens_event_step below.
EVENT_EXPORTS = ["tmg_ens_event_plan", "tmg_ens_event_count", "tmg_ens_event_step"]
# The pooled probability densities: marginal and joint histograms of the members and of the target (csrc/tmg_pdf.hip), declared in
# include/tmglow_hip_pdf.h: ens_pdf_plan / ens_pdf_count below.
PDF_EXPORTS = ["tmg_ens_pdf_plan", "tmg_ens_pdf_count"]
# The projection on the target's POD modes (csrc/tmg_pod.hip), declared in include/tmglow_hip_pod.h: ens_pod_plan / ens_pod_project
# below.
POD_EXPORTS = ["tmg_ens_pod_plan", "tmg_ens_pod_project"]
# The phase averages on the shedding phase (csrc/tmg_phase.hip), declared in include/tmglow_hip_phase.h: ens_phase_plan /
# ens_phase_label / ens_phase_accum below.
PHASE_EXPORTS = ["tmg_ens_phase_plan", "tmg_ens_phase_label", "tmg_ens_phase_accum"]
# The spectral POD: the members' cross-spectral density matrices and the synthesis of the modes (csrc/tmg_spod.hip), declared in
# include/tmglow_hip_spod.h, a header of its own: ens_spod_plan / ens_spod_csd / ens_spod_modes below.
SPOD_EXPORTS = ["tmg_ens_spod_plan", "tmg_ens_spod_csd", "tmg_ens_spod_modes"]
# The layout conversions of the level node's backward pass (csrc/tmg_thin.hip), declared in include/tmglow_hip_layout.h: layer_unplanes below.
LAYOUT_EXPORTS = ["tmg_layer_unplanes"]
# The budget of the turbulent kinetic energy (csrc/tmg_budget.hip), declared in include/tmglow_hip_budget.h, a header of its own:
# ens_budget_plan / ens_budget_accum / ens_budget_terms below.
BUDGET_EXPORTS = ["tmg_ens_budget_plan", "tmg_ens_budget_accum", "tmg_ens_budget_terms"]
# The two-point space-time correlations about probe points (csrc/tmg_corr.hip), declared in include/tmglow_hip_corr.h, a header of its
# own: ens_corr_plan / ens_corr_probe / ens_corr_accum / ens_corr_finalize below.
CORR_EXPORTS = ["tmg_ens_corr_plan", "tmg_ens_corr_probe", "tmg_ens_corr_accum", "tmg_ens_corr_finalize"]
# The scale-to-scale energy flux and the sub-filter stresses (csrc/tmg_flux.hip), declared in include/tmglow_hip_flux.h, a header of its
# own: ens_flux_plan / ens_flux_accum / ens_flux_terms below.
FLUX_EXPORTS = ["tmg_ens_flux_plan", "tmg_ens_flux_accum", "tmg_ens_flux_terms"]
# The Lagrangian transport: pathlines, FTLE, residence time (csrc/tmg_lagr.hip), declared in include/tmglow_hip_lagr.h, a header of its
# own: ens_lagr_plan / ens_lagr_advect / ens_lagr_store / ens_lagr_finalize below.
LAGR_EXPORTS = ["tmg_ens_lagr_plan", "tmg_ens_lagr_advect", "tmg_ens_lagr_store", "tmg_ens_lagr_finalize"]
# The vortex census: Okubo-Weiss classes, connected-component labels, int64 measures (csrc/tmg_vortex.hip), declared in
# include/tmglow_hip_vortex.h, a header of its own: ens_vortex_plan / ens_vortex_classify / ens_vortex_label / ens_vortex_census below.
VORTEX_EXPORTS = ["tmg_ens_vortex_plan", "tmg_ens_vortex_classify", "tmg_ens_vortex_label", "tmg_ens_vortex_census"]
# The multivariate rank histograms: the average-rank and band-depth pre-ranks of every row (csrc/tmg_frank.hip), declared in
# include/tmglow_hip_frank.h, a header of its own: ens_frank_plan / ens_frank_step below.
FRANK_EXPORTS = ["tmg_ens_frank_plan", "tmg_ens_frank_step"]
# The spectral skill: coherence, error and spread spectra against the target (csrc/tmg_xspec.hip), declared in
# include/tmglow_hip_xspec.h, a header of its own: ens_xspec_plan / ens_xspec_prep / ens_xspec_cols / ens_xspec_accum below.
XSPEC_EXPORTS = ["tmg_ens_xspec_plan", "tmg_ens_xspec_prep", "tmg_ens_xspec_cols", "tmg_ens_xspec_accum"]
# The event durations: spells, gaps and persistence along the time window (csrc/tmg_spell.hip), declared in
# include/tmglow_hip_spell.h, a header of its own: ens_spell_plan / ens_spell_step / ens_spell_finalize below.
SPELL_EXPORTS = ["tmg_ens_spell_plan", "tmg_ens_spell_step", "tmg_ens_spell_finalize"]
# The intensity-scale verification: the Haar skill of the events by spatial scale (csrc/tmg_iscale.hip), declared in
# include/tmglow_hip_iscale.h, a header of its own: ens_iscale_plan / ens_iscale_chunk / ens_iscale_step below.
ISCALE_EXPORTS = ["tmg_ens_iscale_plan", "tmg_ens_iscale_chunk", "tmg_ens_iscale_step"]
# The excursion-set morphology: the counts behind the Minkowski functionals of a ladder of levels (csrc/tmg_mink.hip), declared in
# include/tmglow_hip_mink.h, a header of its own: ens_mink_plan / ens_mink_chunk below.
MINK_EXPORTS = ["tmg_ens_mink_plan", "tmg_ens_mink_chunk"]
# The distance-map verification: the exact Euclidean distance transform of the event sets and the sums behind the mean error distance,
# the Hausdorff distances and Baddeley's delta (csrc/tmg_edt.hip), declared in include/tmglow_hip_edt.h, a header of its own:
# ens_edt_plan / ens_edt_chunk / ens_edt_step / ens_edt_fixed below.
EDT_EXPORTS = ["tmg_ens_edt_plan", "tmg_ens_edt_chunk", "tmg_ens_edt_step", "tmg_ens_edt_fixed"]
# The line spectra: 1-D fluctuation, mean-flow and co-spectra along x or y (csrc/tmg_lspec.hip), declared in
# include/tmglow_hip_lspec.h, a header of its own: ens_lspec_plan / ens_lspec_chunk / ens_lspec_step / ens_lspec_finalize below.
LSPEC_EXPORTS = ["tmg_ens_lspec_plan", "tmg_ens_lspec_chunk", "tmg_ens_lspec_step", "tmg_ens_lspec_finalize"]
_P64 = ctypes.POINTER(ctypes.c_int64)
LSPEC_ARGTYPES = {
    "tmg_ens_lspec_plan": [_P64, _P64],
    "tmg_ens_lspec_chunk": [ctypes.c_void_p, _P64] + [ctypes.c_void_p] * 7 + [_P64, ctypes.c_void_p],
    "tmg_ens_lspec_step": [ctypes.c_void_p] * 4 + [_P64, ctypes.c_void_p],
    "tmg_ens_lspec_finalize": [ctypes.c_void_p] * 7 + [_P64, ctypes.c_void_p],
}
FLUX_ARGTYPES = {
    "tmg_ens_flux_plan": [_P64, _P64, _P64],
    "tmg_ens_flux_accum": [ctypes.c_void_p, _P64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, _P64, _P64, ctypes.c_void_p],
    "tmg_ens_flux_terms": [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p, _P64, _P64, ctypes.c_void_p],
}
FRANK_ARGTYPES = {
    "tmg_ens_frank_plan": [_P64, _P64],
    "tmg_ens_frank_step": [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, _P64,
                           ctypes.c_void_p],
}
SPELL_ARGTYPES = {
    "tmg_ens_spell_plan": [_P64, _P64],
    "tmg_ens_spell_step": [ctypes.c_void_p, _P64, ctypes.c_void_p, _P64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, _P64,
                           ctypes.c_void_p],
    "tmg_ens_spell_finalize": [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, _P64, ctypes.c_void_p],
}
ISCALE_ARGTYPES = {
    "tmg_ens_iscale_plan": [_P64, _P64],
    "tmg_ens_iscale_chunk": [ctypes.c_void_p, _P64, ctypes.c_void_p, _P64, ctypes.c_void_p, _P64, ctypes.c_void_p, ctypes.c_void_p,
                             ctypes.c_void_p, ctypes.c_void_p, _P64, ctypes.c_void_p],
    "tmg_ens_iscale_step": [ctypes.c_void_p, ctypes.c_void_p, _P64, ctypes.c_void_p, _P64, ctypes.c_void_p, _P64, ctypes.c_void_p],
}
MINK_ARGTYPES = {
    "tmg_ens_mink_plan": [_P64, _P64],
    "tmg_ens_mink_chunk": [ctypes.c_void_p, _P64, ctypes.c_void_p, _P64, ctypes.c_void_p, _P64, ctypes.c_void_p, _P64, ctypes.c_void_p],
}
EDT_ARGTYPES = {
    "tmg_ens_edt_plan": [_P64, _P64],
    "tmg_ens_edt_chunk": [ctypes.c_void_p, _P64, ctypes.c_void_p, _P64, ctypes.c_void_p, _P64, ctypes.c_void_p, ctypes.c_void_p,
                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, _P64, ctypes.c_void_p],
    "tmg_ens_edt_step": [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, _P64, ctypes.c_void_p],
    "tmg_ens_edt_fixed": [_P64, ctypes.c_int64, ctypes.c_int64, _P64],
}
XSPEC_ARGTYPES = {
    "tmg_ens_xspec_plan": [_P64, _P64],
    "tmg_ens_xspec_prep": [ctypes.c_void_p, _P64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                           ctypes.c_void_p, _P64, ctypes.c_void_p],
    "tmg_ens_xspec_cols": [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, _P64,
                           ctypes.POINTER(ctypes.c_float), ctypes.c_void_p],
    "tmg_ens_xspec_accum": [ctypes.c_void_p] * 10 + [_P64, ctypes.c_void_p],
}
# Every export returns int except the workspace sizes, which the header declares int64_t (read through a 32-bit return a request of
# 2^31 floats or more would be truncated and the kernel handed a buffer smaller than it planned for).
RET_I64 = ("tmg_conv_wgrad_ws_floats", "tmg_conv_wgrad_grouped_ws_floats", "tmg_conv_wino_wgrad_ws_floats",
           "tmg_conv_wino_wgrad_grouped_ws_floats")


def build(force=False, verbose=False):
    """Compile the HIP sources for gfx950 into libtmglow_hip.so (in-tree).  One object per source (recompiled only when the
    source or a header changed, all stale ones in parallel), then one link."""
    from concurrent.futures import ThreadPoolExecutor
    inc = os.path.join(os.path.dirname(_HERE), "include")
    headers = [os.path.join(CSRC, "tmg_common.h"), os.path.join(CSRC, "tmg_symgram.h"), os.path.join(CSRC, "tmg_field.h"), os.path.join(CSRC, "tmg_dft.h"),
               os.path.join(inc, "tmglow_hip.h"), os.path.join(inc, "tmglow_hip_plan.h"),
               os.path.join(inc, "tmglow_hip_tspec.h"), os.path.join(inc, "tmglow_hip_quant.h"),
               os.path.join(inc, "tmglow_hip_gram.h"), os.path.join(inc, "tmglow_hip_sfun.h"),
               os.path.join(inc, "tmglow_hip_event.h"), os.path.join(inc, "tmglow_hip_pdf.h"), os.path.join(inc, "tmglow_hip_pod.h"),
               os.path.join(inc, "tmglow_hip_phase.h"), os.path.join(inc, "tmglow_hip_spod.h"), os.path.join(inc, "tmglow_hip_layout.h"),
               os.path.join(inc, "tmglow_hip_budget.h"), os.path.join(inc, "tmglow_hip_corr.h"), os.path.join(inc, "tmglow_hip_flux.h"),
               os.path.join(inc, "tmglow_hip_lagr.h"), os.path.join(inc, "tmglow_hip_vortex.h"),
               os.path.join(inc, "tmglow_hip_frank.h"), os.path.join(inc, "tmglow_hip_xspec.h"), os.path.join(inc, "tmglow_hip_spell.h"),
               os.path.join(inc, "tmglow_hip_iscale.h"), os.path.join(inc, "tmglow_hip_mink.h"), os.path.join(inc, "tmglow_hip_edt.h"),
               os.path.join(inc, "tmglow_hip_lspec.h")]
    hmt = max(os.path.getmtime(h) for h in headers)
    objdir = os.path.join(_HERE, "build")
    os.makedirs(objdir, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = ["--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-Wno-unused-result", "-I", inc]
    jobs, objs, stamps = [], [], []
    for src in SOURCES:
        sp, ob = os.path.join(CSRC, src), os.path.join(objdir, src.replace(".hip", ".o"))
        objs.append(ob)
        extra = ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"] if src in NO_PACKED_F32 else []
        # an object is stale when its source / a header is newer OR when its flags (kept beside it) are not this build's:
        # an edit of NO_PACKED_F32 or of the flag list recompiles what it changes
        line = " ".join(flags + extra)
        stamp = ob + ".flags"
        old = open(stamp).read() if os.path.exists(stamp) else None
        if force or old != line or not os.path.exists(ob) or os.path.getmtime(ob) < max(os.path.getmtime(sp), hmt):
            jobs.append([hipcc] + flags + extra + ["-c", sp, "-o", ob])
            stamps.append((stamp, line))
    if not jobs and os.path.exists(LIB_PATH) and all(os.path.getmtime(LIB_PATH) >= os.path.getmtime(o) for o in objs):
        return LIB_PATH

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
        # (hipcc hands -target-feature to its HOST pass as well, which prints one "not a recognized feature" line per kernel: dropped)
        err = "\n".join(ln for ln in r.stderr.splitlines() if "'-packed-fp32-ops' is not a recognized feature" not in ln)
        if err.strip():
            print(err, file=sys.stderr, flush=True)
        if r.returncode != 0:
            raise subprocess.CalledProcessError(r.returncode, cmd)

    with ThreadPoolExecutor(max_workers=4) as ex:
        list(ex.map(run, jobs))
    for stamp, line in stamps:
        open(stamp, "w").write(line)
    run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", LIB_PATH])
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libtmglow_hip.so is missing (%s): run `python -c 'import __graft_entry__ as g; g.build()'`. "
                               "There is no fallback path." % LIB_PATH)
        _lib = ctypes.CDLL(LIB_PATH)
        for name in EXPORTS:
            getattr(_lib, name).restype = c_i64 if name in RET_I64 else ctypes.c_int
        _lib.tmg_prof_name.restype = ctypes.c_char_p
        for name in PLAN_EXPORTS:
            getattr(_lib, name).restype = ctypes.c_int
            getattr(_lib, name).argtypes = PLAN_ARGTYPES[name]
        for name in TSPEC_EXPORTS + QUANT_EXPORTS + GRAM_EXPORTS + SFUN_EXPORTS + EVENT_EXPORTS + PDF_EXPORTS + POD_EXPORTS + PHASE_EXPORTS + SPOD_EXPORTS + LAYOUT_EXPORTS + BUDGET_EXPORTS + CORR_EXPORTS + LAGR_EXPORTS + VORTEX_EXPORTS:
            getattr(_lib, name).restype = ctypes.c_int
        for name in FLUX_EXPORTS:
            getattr(_lib, name).restype = ctypes.c_int
            getattr(_lib, name).argtypes = FLUX_ARGTYPES[name]
        for name in FRANK_EXPORTS:
            getattr(_lib, name).restype = ctypes.c_int
            getattr(_lib, name).argtypes = FRANK_ARGTYPES[name]
        for name in XSPEC_EXPORTS:
            getattr(_lib, name).restype = ctypes.c_int
            getattr(_lib, name).argtypes = XSPEC_ARGTYPES[name]
        for name in SPELL_EXPORTS:
            getattr(_lib, name).restype = ctypes.c_int
            getattr(_lib, name).argtypes = SPELL_ARGTYPES[name]
        for name in ISCALE_EXPORTS:
            getattr(_lib, name).restype = ctypes.c_int
            getattr(_lib, name).argtypes = ISCALE_ARGTYPES[name]
        for name in MINK_EXPORTS:
            getattr(_lib, name).restype = ctypes.c_int
            getattr(_lib, name).argtypes = MINK_ARGTYPES[name]
        for name in EDT_EXPORTS:
            getattr(_lib, name).restype = ctypes.c_int
            getattr(_lib, name).argtypes = EDT_ARGTYPES[name]
        for name in LSPEC_EXPORTS:
            getattr(_lib, name).restype = ctypes.c_int
            getattr(_lib, name).argtypes = LSPEC_ARGTYPES[name]
    return _lib


def prof_enable(on):
    """False / 0: off; True / 1: time the matrix-core kernels; 2: also the bandwidth-bound kernel classes."""
    lib().tmg_prof_enable(c_i64(int(on)))


def prof_kernel_id(name):
    """Kernel id of a name returned by prof_collect (for prof_enable(100 + id): time only that kernel)."""
    l = lib()
    for k in range(64):
        if l.tmg_prof_name(c_i64(k)).decode() == name:
            return k
    raise KeyError(name)


def prof_collect():
    """{kernel name: (launches, total ms, total algorithmic work)} of the event-timed kernels: work = flops for the matrix-core
    kernels, HBM bytes for the classes whose name starts with "hbm:"."""
    l = lib()
    nk = 64
    buf = (ctypes.c_double * (3 * nk))()
    n = l.tmg_prof_collect(buf, c_i64(nk))
    out = {}
    for k in range(n):
        if buf[3 * k] > 0:
            out[l.tmg_prof_name(c_i64(k)).decode()] = (int(buf[3 * k]), buf[3 * k + 1], buf[3 * k + 2])
    return out


def _stream():
    """Raw handle of torch's CURRENT stream on the current device.  (torch.cuda.current_stream() builds a Stream object through three
    layers of Python per call - 8 us, once per kernel launch: 3 ms of host time per step; the raw getter is a single C call.)"""
    return c_vp(torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice()))


def _chk(code, name):
    if code != 0:
        raise RuntimeError("%s failed with code %d" % (name, code))


def _ptr(t):
    return c_vp(t.data_ptr()) if t is not None else c_vp(0)


def check_act(t):
    if not (t.is_cuda and t.dtype == torch.float32):
        raise RuntimeError("TM-Glow HIP ops need fp32 tensors on a HIP device (got %s on %s); there is no CPU path"
                           % (t.dtype, t.device))


def seg(t):
    """(ptr, pixel stride, channel offset folded into ptr => 0, n) of an NHWC tensor or channel-slice view."""
    check_act(t)
    B, H, W, C = t.shape
    s = t.stride()
    ps = s[2] if W > 1 else (s[1] // W if H > 1 else (s[0] // (H * W) if B > 1 else C))
    ok = s[3] == 1 or C == 1
    if W > 1:
        ok = ok and (H == 1 or s[1] == W * ps) and (B == 1 or s[0] == H * W * ps)
    if not ok or ps < C:
        raise RuntimeError("tensor is not an NHWC channel-slice: shape %s strides %s" % (tuple(t.shape), s))
    return (t.data_ptr(), int(ps), 0, int(C))


def check_device(t):
    """Kernels launch on the CURRENT device's current stream: a tensor that lives on another GPU would be read through a
    foreign pointer (fault, or silent peer traffic).  The model entry points (TMGlow.forward / sample / reconstruct) switch to
    their input's device themselves; stand-alone modules must be called with their device current."""
    if t.is_cuda and t.device.index != torch.cuda.current_device():
        raise RuntimeError("TM-Glow HIP op called with a tensor on %s while the current device is cuda:%d: wrap the call in "
                           "`with torch.cuda.device(t.device):` (or torch.cuda.set_device once per process)"
                           % (t.device, torch.cuda.current_device()))


def nhwc(x):
    """API tensor [B,C,H,W] (any strides) -> internal [B,H,W,C] contiguous (free if channels_last)."""
    check_act(x)
    check_device(x)
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    """internal [B,H,W,C] -> API-shaped [B,C,H,W] view (channels_last strides)."""
    return t.permute(0, 3, 1, 2)


def _segs(tensors):
    d = [seg(t) for t in tensors]
    ptrs = (c_vp * len(d))(*[x[0] for x in d])
    desc = (c_i64 * (3 * len(d)))(*[v for x in d for v in (x[1], x[2], x[3])])
    return ptrs, desc, len(d)


def _d2(t):
    """{pixel stride, 0} of a tensor (the channel offset of a slice view is already folded into its data pointer); zeros for None
    (an optional operand: its pointer is null and the library does not read the descriptor)."""
    return (c_i64 * 2)(seg(t)[1] if t is not None else 0, 0)


def _i64(*v):
    return (c_i64 * len(v))(*[int(x) for x in v])


def _flts(vals):
    return (ctypes.c_float * len(vals))(*[float(v) for v in vals])


def _launched(rc, name):
    """The envelope convention: -100 = the shape is outside the kernel's envelope and nothing was launched (False); any other
    non-zero code raises."""
    if rc == -100:
        return False
    _chk(rc, name)
    return True


def _packed_numel(mode, ce, Cout, k):
    """Floats of the direct kernels' packed operand (tmg_conv_pack): k k taps of [K -> 16][N -> 16], K x N = ce x Cout (mode 0) or
    Cout x ce (mode 1)."""
    K, N = (ce, Cout) if mode == 0 else (Cout, ce)
    return k * k * ((K + 15) // 16 * 16) * ((N + 15) // 16 * 16)


# ------------------------------------------------------------------------------------------------
# dense contractions
# ------------------------------------------------------------------------------------------------
# Bumped by code that rewrites parameter memory behind torch's version counters (tmg_optim.HipAdam, tmg_dist.broadcast_parameters,
# tmg_ops.invalidate_derived); tmg_ops.PARAM_GENERATION is this list.
PARAM_GENERATION = [0]


class _PackPlan:
    """The packed MFMA operands of the model's PARAMETERS, all re-packed by a few launches per parameter update instead of one
    launch per conv and pass (round 5: 67 tmg_conv_pack launches of ~4.6 us per training step, 670 per eager BPTT window).  The plan
    learns which (parameter, mode, cin_eff, cmap) operands the model asks for; the first request that finds its operand stale - the
    parameter's memory, torch version counter or PARAM_GENERATION moved - re-packs EVERY known operand whose parameter moved
    (tmg_conv_pack_many, 48 jobs per launch), later requests of the same parameter state are dictionary look-ups.  Only nn.Parameter
    objects take part (identity + weak reference): temporaries derived from parameters have no version to check and are packed per call
    as before.  While a hipGraph is being recorded the plan is bypassed (the recorded pass must re-pack at every replay)."""

    def __init__(self):
        self.jobs = {}

    @staticmethod
    def _state(w):
        return (w.data_ptr(), w._version, PARAM_GENERATION[0], w.device)

    def get(self, w, mode, cin_eff, cmap):
        key = (id(w), int(mode), int(cin_eff), cmap)
        e = self.jobs.get(key)
        st = self._state(w)
        if e is not None and e["ref"]() is w and e["state"] == st:
            return e["out"]
        self.jobs[key] = {"ref": weakref.ref(w), "state": None, "out": None, "spec": (int(mode), int(cin_eff), cmap)}
        self._repack(w.device)
        return self.jobs[key]["out"]

    def _repack(self, device):
        todo = []
        for k in list(self.jobs):
            e = self.jobs[k]
            w = e["ref"]()
            if w is None:
                del self.jobs[k]
            elif w.device == device and e["state"] != self._state(w):
                todo.append((e, w))
        outs = conv_pack_many([(w,) + e["spec"] for e, w in todo])
        for (e, w), o in zip(todo, outs):
            e["out"], e["state"] = o, self._state(w)


_PACK_PLAN = _PackPlan()


def conv_pack(w, mode, cin_eff=0, cmap=None):
    """w: torch layout [Cout, Cin, k, k] -> packed MFMA operand (see tmg_conv_pack); cin_eff > Cin zero-extends the
    input-channel dimension.  cmap = (cvalid, csplit, cgap) selects / re-maps source channels (tmg_conv_pack_map).  Parameters go
    through the pack plan (_PackPlan: the returned tensor is shared by every request of the same parameter state - read-only)."""
    check_act(w)
    if (isinstance(w, torch.nn.Parameter) and w.is_contiguous() and os.environ.get("TMG_NO_PACK_PLAN") is None
            and not torch.cuda.is_current_stream_capturing()):
        return _PACK_PLAN.get(w, mode, cin_eff, tuple(int(v) for v in cmap) if cmap is not None else None)
    w = w.contiguous()
    Cout, Cin, k, _ = w.shape
    if cmap is not None:
        ce = int(cin_eff)
        wpk = torch.empty(_packed_numel(mode, ce, Cout, k), device=w.device, dtype=torch.float32)
        _chk(lib().tmg_conv_pack_map(_ptr(w), _ptr(wpk), c_i64(Cout), c_i64(Cin), c_i64(ce), c_i64(k), c_i64(mode), _i64(*cmap), _stream()),
             "tmg_conv_pack_map")
        return wpk
    ce = max(int(cin_eff), Cin)
    wpk = torch.empty(_packed_numel(mode, ce, Cout, k), device=w.device, dtype=torch.float32)
    _chk(lib().tmg_conv_pack(_ptr(w), _ptr(wpk), c_i64(Cout), c_i64(Cin), c_i64(ce), c_i64(k), c_i64(mode), _stream()), "tmg_conv_pack")
    return wpk


def conv_pack_many(jobs):
    """jobs: list of (w, mode) or (w, mode, cin_eff, cmap) as conv_pack takes them -> list of packed operands, <= 48 jobs per launch
    (tmg_conv_pack_many).  All operands of a launch live in one allocation."""
    outs = []
    for g0 in range(0, len(jobs), 48):
        grp = [tuple(j) + (0, None)[len(j) - 2:] for j in jobs[g0:g0 + 48]]
        desc, sizes, ws = [], [], []
        for w, mode, cin_eff, cmap in grp:
            check_act(w)
            assert w.is_contiguous()
            Cout, Cin, k, _ = w.shape
            ce = int(cin_eff) if cmap is not None else max(int(cin_eff), Cin)
            m = cmap if cmap is not None else (Cin, 0x7fffffff, 0)
            desc += [Cout, Cin, ce, k, mode, m[0], m[1], m[2]]
            sizes.append(_packed_numel(mode, ce, Cout, k))
            ws.append(w)
        flat = torch.empty(sum(sizes), device=ws[0].device, dtype=torch.float32)
        views, o = [], 0
        for n_ in sizes:
            views.append(flat[o:o + n_])
            o += n_
        wp = (c_vp * len(ws))(*[w.data_ptr() for w in ws])
        op = (c_vp * len(ws))(*[v.data_ptr() for v in views])
        _chk(lib().tmg_conv_pack_many(wp, op, _i64(*desc), c_i64(len(ws)), _stream()), "tmg_conv_pack_many")
        outs += views
    return outs


def conv_pack_batched(w, mode, cin_eff=0, cmap=None):
    """w: [N, Cout, Cin, k, k] -> [N, packed] (one launch); arguments as conv_pack."""
    check_act(w)
    w = w.contiguous()
    N_, Cout, Cin, k, _ = w.shape
    ce = int(cin_eff) if cmap is not None else max(int(cin_eff), Cin)
    wpk = torch.empty((N_, _packed_numel(mode, ce, Cout, k)), device=w.device, dtype=torch.float32)
    m = cmap if cmap is not None else (Cin, 0x7fffffff, 0)
    _chk(lib().tmg_conv_pack_batched(_ptr(w), _ptr(wpk), c_i64(N_), c_i64(Cout), c_i64(Cin), c_i64(ce), c_i64(k), c_i64(mode), _i64(*m),
                                     _stream()), "tmg_conv_pack_batched")
    return wpk


def conv_fwd(inputs, wpk, Cout, ksize, stride, outs, bias=None, kappa=None, in_scale=None, in_shift=None, relu_in=False,
             pad_rep=False, relu_out=False, accumulate=False, add=None):
    """inputs / outs: lists of NHWC tensors (or channel-slice views) forming the channel concatenation.
    add: optional NHWC tensor / channel-slice view with Cout channels summed in before bias and scale."""
    B, Hin, Win, _ = inputs[0].shape
    Hout, Wout = outs[0].shape[1], outs[0].shape[2]
    ip, idesc, n_in = _segs(inputs)
    op, odesc, n_out = _segs(outs)
    Cin = sum(t.shape[3] for t in inputs)
    assert sum(t.shape[3] for t in outs) == Cout
    dims = _i64(B, Hin, Win, Hout, Wout, ksize, stride, Cin, Cout, relu_in, pad_rep, relu_out, accumulate)
    if add is not None:
        _chk(lib().tmg_conv_fwd_add(ip, idesc, c_i64(n_in), _ptr(wpk), _ptr(bias), _ptr(kappa), _ptr(in_scale), _ptr(in_shift), _ptr(add),
                                    _d2(add), op, odesc, c_i64(n_out), dims, _stream()), "tmg_conv_fwd_add")
        return
    _chk(lib().tmg_conv_fwd(ip, idesc, c_i64(n_in), _ptr(wpk), _ptr(bias), _ptr(kappa), _ptr(in_scale), _ptr(in_shift), op, odesc,
                            c_i64(n_out), dims, _stream()), "tmg_conv_fwd")


def wino_eligible(Cin, Cout, ksize, stride):
    """Shapes the Winograd F(2x2, 3x3) kernel takes over from the direct implicit GEMM: 3x3 / stride 1 with many output
    channels (the matrix-pipe-bound contractions)."""
    return ksize == 3 and stride == 1 and Cout >= 64 and Cout % 4 == 0 and Cin % 4 == 0 and Cin >= 16


def wino_narrow_eligible(Cin, Cout):
    """Shapes of the few-output-channel Winograd kernel (the input gradients of the wide contractions, the ConvLSTM block's
    narrow convs): 3x3 / stride 1, Cout <= 48, Cin >= 64."""
    return Cout <= 48 and Cout % 4 == 0 and Cin % 4 == 0 and Cin >= 64


def conv_wino_pack(w, mode=0, nvalid=0):
    """Winograd operand U = G g G^T of a [Cout, Cin, 3, 3] weight: [16][K_pad/16][N_pad][16] floats.  mode 0: forward (K = Cin,
    N = Cout); mode 1: input gradient w.r.t. the first `nvalid` input channels (K = Cout, N = nvalid or Cin), taps flipped."""
    Cout, Cin = w.shape[0], w.shape[1]
    assert w.shape[2] == 3 and w.shape[3] == 3
    w = w.contiguous()
    K, N = (Cin, Cout) if mode == 0 else (Cout, nvalid if 0 < nvalid < Cin else Cin)
    U = torch.empty(16 * ((K + 15) // 16 * 16) * ((N + 15) // 16 * 16), device=w.device, dtype=torch.float32)
    _chk(lib().tmg_conv_wino_pack(_ptr(w), _ptr(U), c_i64(Cout), c_i64(Cin), c_i64(mode), c_i64(nvalid), _stream()), "tmg_conv_wino_pack")
    return U


# Arithmetic of the WIDE Winograd contractions (conv3x3_auto): "f32" = fp32 MFMA (the default, the headline's); "bf16x3" = the bf16
# matrix pipe at fp32 accuracy (three-way exact split of both operands, six part products: tmg_conv_wino_fwd3) - opt-in
_WINO_PRECISION = ["bf16x3" if os.environ.get("TMG_WINO_BF3") else "f32"]


def set_winograd_precision(kind):
    if kind not in ("f32", "bf16x3"):
        raise ValueError("Winograd precision must be 'f32' or 'bf16x3', got %r" % (kind,))
    _WINO_PRECISION[0] = kind


def winograd_precision():
    return _WINO_PRECISION[0]


def conv_wino_pack3(w, mode=0, nvalid=0):
    """bf16x3 Winograd operand of a [Cout, Cin, 3, 3] weight (tmg_conv_wino_pack3): U = G g G^T in fp32, split into three bf16 parts,
    in A-fragment order of mfma_f32_16x16x32_bf16.  Modes as conv_wino_pack."""
    Cout, Cin = w.shape[0], w.shape[1]
    assert w.shape[2] == 3 and w.shape[3] == 3
    w = w.contiguous()
    K, N = (Cin, Cout) if mode == 0 else (Cout, nvalid if 0 < nvalid < Cin else Cin)
    U = torch.empty(16 * ((K + 31) // 32 * 32) * ((N + 15) // 16 * 16) * 3, device=w.device, dtype=torch.int16)
    _chk(lib().tmg_conv_wino_pack3(_ptr(w), _ptr(U), c_i64(Cout), c_i64(Cin), c_i64(mode), c_i64(nvalid), _stream()), "tmg_conv_wino_pack3")
    return U


def _wino_fwd(name, inputs, U, Cout, outs, bias, *flags):
    """The three Winograd forwards: same marshalling, dims = {B, H, W, Cin, Cout, flags..}."""
    if isinstance(outs, torch.Tensor):
        outs = [outs]
    B, Hin, Win, _ = inputs[0].shape
    ip, idesc, n_in = _segs(inputs)
    op, odesc, n_out = _segs(outs)
    Cin = sum(t.shape[3] for t in inputs)
    assert sum(t.shape[3] for t in outs) == Cout and outs[0].shape[1] == Hin and outs[0].shape[2] == Win
    return _launched(getattr(lib(), name)(ip, idesc, c_i64(n_in), _ptr(U), _ptr(bias), op, odesc, c_i64(n_out),
                                          _i64(B, Hin, Win, Cin, Cout, *flags), _stream()), name)


def conv_wino_fwd3(inputs, U, Cout, outs, bias=None, relu_in=False, pad_rep=False):
    """conv_wino_fwd with the bf16x3 operand of conv_wino_pack3; False outside the envelope (nothing was launched)."""
    return _wino_fwd("tmg_conv_wino_fwd3", inputs, U, Cout, outs, bias, relu_in, pad_rep)


def conv_wino_narrow(inputs, U, Cout, outs, bias=None, relu_in=False, pad_rep=False, relu_out=False):
    """Few output channels: outs = list of <= 3 NHWC tensors / channel-slice views forming the Cout channels.  False when the
    shape is outside the kernel's envelope (nothing was launched)."""
    return _wino_fwd("tmg_conv_wino_narrow", inputs, U, Cout, outs, bias, relu_in, pad_rep, relu_out)


def conv_wino_fwd(inputs, U, Cout, outs, bias=None, relu_in=False, pad_rep=False):
    """outs = conv3x3(pad(act(cat(inputs)))) + bias through the Winograd kernel (outs: tensor or list of <= 3 segments); False when
    the shape is outside its envelope (nothing was launched: the caller runs conv_fwd with the direct operand)."""
    return _wino_fwd("tmg_conv_wino_fwd", inputs, U, Cout, outs, bias, relu_in, pad_rep)


def conv3x3_auto(inputs, weight, Cout, outs, bias=None, relu_in=False, pad_rep=False, relu_out=False, dgrad=False, nvalid=0):
    """A plain 3x3 / stride-1 contraction (no kappa / add / accumulate) through the fastest kernel that takes the shape: Winograd
    (wide or narrow) when eligible, the direct implicit GEMM otherwise.  dgrad: the input gradient of a conv with this weight
    ([K = weight.shape[0] dy channels] -> the first `nvalid` (0: all) input channels).  Returns the direct mode-1 operand when it
    had to pack one (callers of replicate-padded convs reuse it for the border fold), else None."""
    Cin = sum(t.shape[3] for t in inputs)
    mode = 1 if dgrad else 0
    if not relu_out and wino_eligible(Cin, Cout, 3, 1):
        # bf16x3 (opt-in): when its kernel declines the shape, the fp32 wide Winograd kernel is next - not the narrow / direct ones
        # (a silent slowdown)
        if (_WINO_PRECISION[0] == "bf16x3"
                and conv_wino_fwd3(inputs, conv_wino_pack3(weight, mode, nvalid), Cout, outs, bias=bias, relu_in=relu_in, pad_rep=pad_rep)):
            return None
        if conv_wino_fwd(inputs, conv_wino_pack(weight, mode, nvalid), Cout, outs, bias=bias, relu_in=relu_in, pad_rep=pad_rep):
            return None
    if wino_narrow_eligible(Cin, Cout):
        if conv_wino_narrow(inputs, conv_wino_pack(weight, mode, nvalid), Cout, outs, bias=bias, relu_in=relu_in, pad_rep=pad_rep,
                            relu_out=relu_out):
            return None
    wpk = conv_pack(weight, mode, nvalid, (nvalid, 1 << 30, 0)) if (dgrad and nvalid) else conv_pack(weight, mode)
    conv_fwd(inputs, wpk, Cout, 3, 1, outs, bias=bias, relu_in=relu_in, pad_rep=pad_rep, relu_out=relu_out)
    return wpk


_WS = {}


def workspace(nfloats, device):
    """Grow-only scratch buffer per (device, stream): kernels on one stream run in order, so sharing it is safe."""
    if torch.cuda.is_current_stream_capturing():
        # a captured launch must not write into a buffer that a later eager call may outgrow and free: scratch of the graph's own pool
        return torch.empty(max(int(nfloats), 1), device=device, dtype=torch.float32)
    key = (device.index, torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice()))
    buf = _WS.get(key)
    if buf is None or buf.numel() < nfloats:
        buf = torch.empty(max(int(nfloats), 1 << 20), device=device, dtype=torch.float32)
        _WS[key] = buf
    return buf


# conv_wgrad's Winograd routing of the 3x3 contractions with 32 - 127 output channels: at least this many input channels and pixels
_WINO_WGRAD_CIN_MIN = 32
_WINO_WGRAD_PIX_MIN = 1 << 20


def conv_wgrad(inputs, dy, dW, dbias, ksize, stride, kappa=None, in_scale=None, in_shift=None, relu_in=False, pad_rep=False,
               use_ws=True, cin_dst=0, cin_valid=0, ci_split=0, ci_off0=0, ci_off1=0):
    B, Hin, Win, _ = inputs[0].shape
    _, Hout, Wout, Cout = dy.shape
    ip, idesc, n_in = _segs(inputs)
    Cin = sum(t.shape[3] for t in inputs)
    if (ksize == 3 and stride == 1 and kappa is None and in_scale is None and use_ws and Cin >= 32
            and (Cout >= 128 or (Cout >= 32 and Cin >= _WINO_WGRAD_CIN_MIN and B * Hin * Win >= _WINO_WGRAD_PIX_MIN))
            # Winograd F(3x3, 2x2), 2.25x fewer matrix-core operations.  Measured per call site at config M: it wins wherever the
            # contraction is matrix-pipe bound (many output channels, or many pixels x input channels) and loses to the direct kernel
            # on the small ones (its 16-position slabs make the reduce step the larger part)
            and conv_wino_wgrad(inputs, dy, dW, dbias, relu_in, pad_rep, cin_dst, cin_valid, ci_split, ci_off0, ci_off1)):
        return
    dims = _i64(B, Hin, Win, Hout, Wout, ksize, stride, Cin, Cout, relu_in, pad_rep, cin_dst, cin_valid, ci_split, ci_off0, ci_off1)
    ws = workspace(lib().tmg_conv_wgrad_ws_floats(dims), dy.device) if use_ws else None
    _chk(lib().tmg_conv_wgrad(ip, idesc, c_i64(n_in), _ptr(in_scale), _ptr(in_shift), _ptr(dy), _d2(dy), _ptr(dW), _ptr(dbias),
                              _ptr(kappa), _ptr(ws), c_i64(ws.numel() if ws is not None else 0), dims, _stream()), "tmg_conv_wgrad")


def wino_wgrad_eligible(Cin, Cout):
    """conv_wgrad's routing rule for the Winograd weight-gradient kernel at large pixel counts (see conv_wgrad)."""
    return Cin >= 32 and Cout >= 128


def conv_wino_wgrad(inputs, dy, dW, dbias, relu_in=False, pad_rep=False, cin_dst=0, cin_valid=0, ci_split=0, ci_off0=0, ci_off1=0):
    """3x3 / stride-1 weight gradient as Winograd F(3x3, 2x2) (tmg_conv_wino_wgrad); False when the shape is outside the kernel's
    envelope (nothing was launched).  conv_wgrad routes the large contractions here."""
    B, Hin, Win, _ = inputs[0].shape
    Cout = dy.shape[3]
    ip, idesc, n_in = _segs(inputs)
    Cin = sum(t.shape[3] for t in inputs)
    wd = _i64(B, Hin, Win, Cin, Cout, relu_in, pad_rep, cin_dst, cin_valid, ci_split, ci_off0, ci_off1)
    need = lib().tmg_conv_wino_wgrad_ws_floats(wd)
    if need > 0:
        ws = workspace(need, dy.device)
        rc = lib().tmg_conv_wino_wgrad(ip, idesc, c_i64(n_in), _ptr(dy), _d2(dy), _ptr(dW), _ptr(dbias), _ptr(ws), c_i64(ws.numel()), wd, _stream())
        if _launched(rc, "tmg_conv_wino_wgrad"):
            return True
    return False


_GTAB = {}


def _segment_table(rows, device):
    """Device copy of a pointer table (the grouped launches' segment tables, tmg_level_pack's parameter table).  The values travel as
    the ARGUMENTS of a fill kernel (tmg_fill_i64, 256 int64 per launch): asynchronous, in stream order, legal during hipGraph capture.
    Round 5 copied the table from pageable host memory on a cache miss - a synchronising copy: one per grouped launch whenever the
    activations' addresses changed, i.e. on every time-step of an eager BPTT window (its T sets of activations are all alive), and with
    round 6's parameter tables in the FORWARD pass it cost the host-bound eager window its run-ahead (0.49 -> 0.53 s per window).
    In a steady single-step loop the caching allocator hands out the same blocks step after step: the table recurs and its device copy
    is reused (no launch at all).  The cache is bounded; a miss is one or two 3-us launches."""
    flat = [int(v) for r in rows for v in r]
    if torch.cuda.is_current_stream_capturing():
        # not cached: the table lives in the graph's pool like every other tensor of the capture
        t = torch.empty((len(rows), len(rows[0])), dtype=torch.int64, device=device)
        _chk(lib().tmg_fill_i64(_ptr(t), _i64(*flat), c_i64(len(flat)), _stream()), "tmg_fill_i64")
        return t
    key = (device.index, len(rows), tuple(flat))
    t = _GTAB.get(key)
    if t is None:
        if len(_GTAB) > 1024:
            _GTAB.clear()
        t = torch.empty((len(rows), len(rows[0])), dtype=torch.int64, device=device)
        _chk(lib().tmg_fill_i64(_ptr(t), _i64(*flat), c_i64(len(flat)), _stream()), "tmg_fill_i64")
        _GTAB[key] = t
    return t


def layer_planes(src):
    """[B,H,W,2K] contiguous -> [K,B,H,W,2]: one pixel-contiguous float2 plane per layer (tmg_layer_planes)."""
    B, Hh, Ww, CP = src.shape
    assert src.is_contiguous() and CP % 4 == 0
    dst = torch.empty((CP // 2, B, Hh, Ww, 2), device=src.device, dtype=torch.float32)
    _chk(lib().tmg_layer_planes(_ptr(src), _ptr(dst), c_i64(B * Hh * Ww), c_i64(CP), _stream()), "tmg_layer_planes")
    return dst


def layer_unplanes(planes, CP):
    """[K,B,H,W,2] contiguous -> [B,H,W,CP] with channel 2k / 2k+1 = plane k and the channels from 2K on zero (tmg_layer_unplanes)."""
    K, B, Hh, Ww, two = planes.shape
    assert planes.is_contiguous() and two == 2 and CP % 4 == 0 and 2 * K <= CP
    dst = torch.empty((B, Hh, Ww, CP), device=planes.device, dtype=torch.float32)
    _chk(lib().tmg_layer_unplanes(_ptr(planes), _ptr(dst), c_i64(B * Hh * Ww), c_i64(CP), c_i64(K), _stream()), "tmg_layer_unplanes")
    return dst


def _pixel_linear(t):
    """[B,H,W,c] view whose pixels are equally spaced in memory (address = base + pixel index * stride(2) + channel)."""
    B, Hh, Ww, _ = t.shape
    return t.stride(3) == 1 and (Hh == 1 or t.stride(1) == t.stride(2) * Ww) and (B == 1 or t.stride(0) == t.stride(2) * Ww * Hh)


def _group_rows(group_inputs, group_dy=None):
    """Rows of the grouped launches' device table: per group 3 input segments {pointer incl. the view's channel offset, pixel stride, 0,
    channels} (unused ones zero), then the group's own upstream gradient {pointer, pixel stride, pointer 2, pixel stride 2}: zeros
    without one, the second pair zero for ONE tensor, both filled for a (half 1, half 2) pair."""
    first = group_inputs[0]
    n_in = len(first)
    dy_pairs = group_dy is not None and isinstance(group_dy[0], (tuple, list))
    rows = []
    for segs in group_inputs:
        # same shapes in every group; the pixel strides may differ (a group's row of the device table carries its own: the first and
        # last layer of a level's node address channel-slice views of [.., C] tensors, the others [.., C/2] tensors of their own)
        assert len(segs) == n_in and all(a.shape == b.shape and a.stride(2) % 4 == b.stride(2) % 4 for a, b in zip(segs, first))
        row = []
        for t in segs:
            row += list(seg(t))  # (pointer incl. the view's channel offset, pixel stride, 0, channels)
        row += [0, 0, 0, 0] * (3 - n_in)
        if group_dy is None:
            row += [0, 0, 0, 0]
        elif dy_pairs:
            a, b = group_dy[len(rows)]
            row += [seg(a)[0], seg(a)[1], seg(b)[0], seg(b)[1]]
        else:
            row += [seg(group_dy[len(rows)])[0], seg(group_dy[len(rows)])[1], 0, 0]
        rows.append(row)
    return rows


def conv_wgrad_thin_grouped(group_inputs, dy, dy_group_channels, dW, relu_in=False, gtab=None, dy_planes=False):
    """The thin grouped 3x3 weight gradient (tmg_conv_wgrad_thin_grouped) called directly: group_inputs[g] a list of <= 3 NHWC
    segments, dy the shared upstream gradient with dy_group_channels (4 or 2) channels per group, dW [G, 4, Cin, 3, 3] accumulated
    into.  dy_planes: dy is [G,B,H,W,2] contiguous, one float2 plane per group.
    Returns the library's code: 0 launched, -100 outside the kernel's envelope (nothing launched)."""
    first = group_inputs[0]
    B, Hin, Win, _ = first[0].shape
    dyc, dys = int(dy_group_channels), dy.stride(-2)
    if dy_planes:
        assert dy.is_contiguous() and dy.shape == (len(group_inputs), B, Hin, Win, 2) and dyc == 2
        dyc = dy.stride(0)      # the distance between two planes takes the place of the channel count (see thin_impl)
        if dyc <= 4:
            return -100
    # the part of the envelope the library cannot see (the segments' addresses live in the device table): float4-addressable pixels
    if not all(t.stride(2) % 4 == 0 and t.data_ptr() % 16 == 0 for segs in group_inputs for t in segs):
        return -100
    if gtab is None:
        gtab = _segment_table(_group_rows(group_inputs), dy.device)
    return lib().tmg_conv_wgrad_thin_grouped(_ptr(gtab), c_i64(len(group_inputs)), _i64(*[t.shape[3] for t in first]), c_i64(len(first)),
                                             _ptr(dy), c_i64(dys), _ptr(dW),
                                             _i64(B, Hin, Win, sum(t.shape[3] for t in first), relu_in, dyc), _stream())


def mix_wgrad_grouped(group_inputs, group_dy, dW, dbias, gtab=None):
    """The streaming weight gradient of the 1x1 mixes (tmg_mix_wgrad_grouped) called directly: group_dy[g] one [B,H,W,C] tensor or a
    (half 1, half 2) pair per group; dW [G, C, C] and dbias [G, C] (or None) accumulated into.  Returns the library's code: 0 launched,
    -100 outside the kernel's envelope (nothing launched)."""
    first = group_inputs[0]
    B, Hin, Win, _ = first[0].shape
    pairs = isinstance(group_dy[0], (tuple, list))
    assert all(_pixel_linear(t) for segs in group_inputs for t in segs)
    assert all(_pixel_linear(t) for e in group_dy for t in (e if pairs else (e,)))
    if gtab is None:
        gtab = _segment_table(_group_rows(group_inputs, group_dy), dW.device)
    return lib().tmg_mix_wgrad_grouped(_ptr(gtab), c_i64(len(group_inputs)), _ptr(dW), _ptr(dbias),
                                       _i64(B * Hin * Win, sum(t.shape[3] for t in first)), _stream())


def conv_wgrad_grouped(group_inputs, dy, dy_group_channels, dW, dbias, ksize, stride, relu_in=False, pad_rep=False, cin_dst=0,
                       cin_valid=0, ci_split=0, ci_off0=0, ci_off1=0, group_dy=None):
    """One launch for len(group_inputs) identically shaped weight gradients.  group_inputs[g]: list of <= 3 NHWC segments;
    dy: [B,H,W,>= G*Cg] with group g at channels [g*Cg, (g+1)*Cg), or None with group_dy = list of G tensors [B,H,W,Cg]
    of identical layout; dW: [G, Cg, cin_dst, k, k] contiguous; dbias: [G, Cg] or None.  Returns False when the library
    cannot group this shape (nothing was launched)."""
    dy_pairs = group_dy is not None and isinstance(group_dy[0], (tuple, list))     # every group's dy as (half 1, half 2) tensors
    if dy_pairs:
        # only the streaming 1x1 kernel below reads an upstream gradient in two halves
        if not (ksize == 1 and stride == 1 and int(dy_group_channels) in (16, 32) and os.environ.get("TMG_NO_MIX_WGRAD_KERNEL") is None):
            group_dy = [torch.cat(list(t), 3) for t in group_dy]
            dy_pairs = False
    if dy is None:
        dy = group_dy[0][0] if dy_pairs else group_dy[0]
        if dy_pairs:
            assert all(a.shape == dy.shape and b.shape == dy.shape for a, b in group_dy)     # (strides per group: from the table)
        else:
            assert all(t.shape == dy.shape and t.stride() == dy.stride() for t in group_dy)
    G = len(group_inputs)
    first = group_inputs[0]
    B, Hin, Win, _ = first[0].shape
    _, Hout, Wout, _ = dy.shape
    Cg = int(dy_group_channels)
    ip, idesc, n_in = _segs(first)
    Cin = sum(t.shape[3] for t in first)
    gtab = _segment_table(_group_rows(group_inputs, group_dy), dy.device)
    if group_dy is None and ksize == 3 and stride == 1 and Cin >= 20 and Cg >= 32:
        # the wide levels' per-layer zero-conv weight gradients: Winograd F(3x3, 2x2), all layers of the level in one launch
        wd = _i64(B, Hin, Win, Cin, Cg, relu_in, pad_rep, cin_dst, cin_valid, ci_split, ci_off0, ci_off1)
        need = lib().tmg_conv_wino_wgrad_grouped_ws_floats(wd, c_i64(G))
        if need > 0:
            ws = workspace(need, dy.device)
            gd = _i64(Cg, dW[0].numel(), dbias[0].numel() if dbias is not None else 0)
            rc = lib().tmg_conv_wino_wgrad_grouped(ip, idesc, c_i64(n_in), _ptr(gtab), c_i64(G), gd, _ptr(dy), _d2(dy), _ptr(dW), _ptr(dbias),
                                                   _ptr(ws), c_i64(ws.numel()), wd, _stream())
            if _launched(rc, "tmg_conv_wino_wgrad_grouped"):
                return True
    if (group_dy is not None and ksize == 1 and stride == 1 and Cg == Cin and Cin in (16, 32) and cin_dst in (0, Cin)
            and cin_valid in (0, Cin) and ci_split == 0 and os.environ.get("TMG_NO_MIX_WGRAD_KERNEL") is None
            and all(_pixel_linear(t) for segs in group_inputs for t in segs)
            and all(_pixel_linear(t) for e in group_dy for t in (e if dy_pairs else (e,)))):
        # the 1x1 mixes' weight gradients: streaming GEMM over the pixels, operands straight from global memory
        rc = mix_wgrad_grouped(group_inputs, group_dy, dW, dbias, gtab=gtab)
        if _launched(rc, "tmg_mix_wgrad_grouped"):
            return True
    if dy_pairs:    # outside the streaming kernel's envelope after all: the general kernels read one tensor per group
        return conv_wgrad_grouped(group_inputs, None, dy_group_channels, dW, dbias, ksize, stride, relu_in=relu_in, pad_rep=pad_rep,
                                  cin_dst=cin_dst, cin_valid=cin_valid, ci_split=ci_split, ci_off0=ci_off0, ci_off1=ci_off1,
                                  group_dy=[torch.cat(list(t), 3) for t in group_dy])
    if (group_dy is None and ksize == 3 and stride == 1 and Cg in (2, 4) and dW.shape[1] == 4 and not pad_rep and dbias is None and cin_dst in (0, Cin)
            and cin_valid in (0, Cin) and ci_split == 0 and Cin in (12, 20, 36, 68) and os.environ.get("TMG_NO_THIN_WGRAD") is None
            and all(t.stride(2) % 4 == 0 and t.data_ptr() % 16 == 0 for segs in group_inputs for t in segs)):
        # four output rows per group (the growth-1 layers; dy: (dd1, dd2, 0, 0) quads or compact (dd1, dd2) pairs): 4x4x1 MFMA blocks
        # instead of 16x16 tiles that would be 2/16 used
        rc = conv_wgrad_thin_grouped(group_inputs, dy, Cg, dW, relu_in=relu_in, gtab=gtab)
        if _launched(rc, "tmg_conv_wgrad_thin_grouped"):
            return True
    dims = _i64(B, Hin, Win, Hout, Wout, ksize, stride, Cin, Cg, relu_in, pad_rep, cin_dst, cin_valid, ci_split, ci_off0, ci_off1)
    ws = workspace(lib().tmg_conv_wgrad_grouped_ws_floats(dims, c_i64(G)), dy.device)
    gd = _i64(Cg, dW[0].numel(), dbias[0].numel() if dbias is not None else 0)
    rc = lib().tmg_conv_wgrad_grouped(ip, idesc, c_i64(n_in), _ptr(gtab), c_i64(G), gd, _ptr(dy), _d2(dy), _ptr(dW), _ptr(dbias),
                                      _ptr(ws), c_i64(ws.numel()), dims, _stream())
    return _launched(rc, "tmg_conv_wgrad_grouped")


def _halves(t):
    """(half 1, half 2) of an activation given as ONE [B,H,W,C] tensor (channel-slice views of it) or as a pair of [B,H,W,C/2]
    tensors (the split layout of the narrow levels)."""
    if isinstance(t, (tuple, list)):
        a, b = t
        assert a.shape == b.shape
        return a, b
    ch = t.shape[3] // 2
    return t[..., :ch], t[..., ch:]


def coupling_fwd(x, out, rsave, y2save, D, hc, wz, bz, kappa, Wm, bm, logdet, reverse, wz_d1col):
    """Zero conv + affine coupling + log-det (+ trailing channel mix) of one coupling layer in one launch (tmg_coupling_fwd_halves).
    x / out: [B,H,W,C] NHWC (or channel-slice views), or PAIRS of [B,H,W,C/2] tensors (channel halves in tensors of their own);
    D: [B,H,W,4] from c1x2_fwd; hc: [B,H,W,C] view of the level's conditioning contribution.  Returns False when the shape is
    outside the kernel's envelope (nothing was launched)."""
    x1, x2 = _halves(x)
    o1, o2 = _halves(out)
    B, Hh, Ww, ch = x1.shape
    s1, s2, t1, t2, sh = seg(x1), seg(x2), seg(o1), seg(o2), seg(hc)
    assert rsave.is_contiguous() and D.is_contiguous() and (y2save is None or y2save.is_contiguous()) and wz.is_contiguous()
    dims = _i64(B, Hh, Ww, 2 * ch, 1 if reverse else 0, s1[1], t1[1], sh[1], wz.shape[1], wz_d1col, s2[1], t2[1])
    rc = lib().tmg_coupling_fwd_halves(c_vp(s1[0]), c_vp(s2[0]), c_vp(t1[0]), c_vp(t2[0]), _ptr(rsave), _ptr(y2save), _ptr(D), c_vp(sh[0]),
                                       _ptr(wz), _ptr(bz), _ptr(kappa), _ptr(Wm), _ptr(bm), _ptr(logdet), dims, _stream())
    return _launched(rc, "tmg_coupling_fwd_halves")


def coupling_bwd(dout, x2, r, g, Wm, wz, kappa, DH, dtin, G0, GD, wz_d1col, fwd=False, x1=None):
    """Mix input gradient + affine-coupling backward + zero-conv input gradient (exact replicate adjoint) of one generative-
    direction coupling layer in one launch (tmg_coupling_bwd_halves).  dout / dtin: [B,H,W,C] tensors or pairs of [B,H,W,C/2] halves;
    x2: the SECOND half of the layer input [B,H,W,C/2] (a channel-slice view or a tensor of its own); DH: [B,H,W,C] channel-slice
    view of the level's stash.  fwd=True: the density direction's layer (mix -> coupling): dout = gradient w.r.t. the coupling
    output, x2 = second half of the coupling OUTPUT, no mix in front (Wm is not read).
    G0=None: the summed form - the first half of dtin receives dto1 + [x1 > 0] G0 and GD = (d d1, d d2, mask bits, 0) for
    dense2_bwd(.., g0_masked=True); x1 [B,H,W,C/2]: the first half of the layer input (a view or a tensor of its own)."""
    d1, d2 = _halves(dout)
    t1, t2 = _halves(dtin)
    B, Hh, Ww, ch = d1.shape
    assert x2.shape[3] == ch
    sd1, sd2, sx, sh, st1, st2 = seg(d1), seg(d2), seg(x2), seg(DH), seg(t1), seg(t2)
    assert r.is_contiguous() and GD.is_contiguous() and Wm.is_contiguous() and wz.is_contiguous()
    assert (G0 is None) != (x1 is None), "the summed form (G0=None) reads x1, the separate form does not"
    dims = [B, Hh, Ww, 2 * ch, sd1[1], sx[1], sh[1], st1[1], wz.shape[1], wz_d1col, sd2[1], st2[1], 1 if fwd else 0]
    if G0 is None:
        assert x1.shape[3] == ch
        dims += list(seg(x1)[:2])
    else:
        assert G0.is_contiguous()
    dims = _i64(*dims)
    rc = lib().tmg_coupling_bwd_halves(c_vp(sd1[0]), c_vp(sd2[0]), c_vp(sx[0]), _ptr(r), _ptr(g), _ptr(Wm), _ptr(wz), _ptr(kappa), c_vp(sh[0]),
                                       c_vp(st1[0]), c_vp(st2[0]), _ptr(G0), _ptr(GD), dims, _stream())
    return _launched(rc, "tmg_coupling_bwd_halves")


def mix_f16(x, W, bias, y, transposed=False):
    """y = fp16(W) . fp16(x) + bias per pixel, fp32 accumulation (tmg_mix_f16); W: fp32 [C, C]; transposed: apply W^T."""
    B, Hh, Ww, C = x.shape
    check_act(W)
    assert W.is_contiguous() and W.shape == (C, C) and y.shape == x.shape
    _chk(lib().tmg_mix_f16(_ptr(x), _d2(x), _ptr(W), _ptr(bias), _ptr(y), _d2(y), _i64(B * Hh * Ww, C, 1 if transposed else 0), _stream()),
         "tmg_mix_f16")


def mat_inverse(W, b=None):
    """(W^-1, -W^-1 b) of K channel mixes [K, C, C] / [K, C] (fp64 arithmetic on the device, rounded once; C <= 64)."""
    K, C = W.shape[0], W.shape[1]
    W = W.contiguous()
    Winv = torch.empty_like(W)
    binv = torch.empty((K, C), device=W.device, dtype=torch.float32) if b is not None else None
    _chk(lib().tmg_mat_inverse(_ptr(W), _ptr(b.contiguous() if b is not None else None), _ptr(Winv), _ptr(binv), _i64(K, C), _stream()),
         "tmg_mat_inverse")
    return Winv, binv


def lu_fold_fwd(tab, sign_s, perm, iperm, W, Wm, bm, ld, reverse, sgn, hw):
    K, C = sign_s.shape
    assert W.dtype == torch.float64 and C <= 256
    _chk(lib().tmg_lu_fold_fwd(_ptr(tab), _ptr(sign_s), _ptr(perm), _ptr(iperm), _ptr(W), _ptr(Wm), _ptr(bm), _ptr(ld), _i64(K, C, reverse),
                               _flts([sgn, hw]), _stream()), "tmg_lu_fold_fwd")


def lu_fold_bwd(tab, sign_s, perm, iperm, W, dWm, dbm, dld, dl, du, dlogs, da, db, reverse, sgn, hw, dWm_tail=None, dbm_tail=None):
    """dWm_tail / dbm_tail: upstream gradients of the LAST layer in tensors of their own (dWm / dbm then cover layers 0..K-2)."""
    K, C = sign_s.shape
    _chk(lib().tmg_lu_fold_bwd_split(_ptr(tab), _ptr(sign_s), _ptr(perm), _ptr(iperm), _ptr(W), _ptr(dWm), _ptr(dbm), _ptr(dWm_tail),
                                     _ptr(dbm_tail), _ptr(dld), _ptr(dl), _ptr(du), _ptr(dlogs), _ptr(da), _ptr(db), _i64(K, C, reverse),
                                     _flts([sgn, hw]), _stream()), "tmg_lu_fold_bwd_split")


def level_finish(Wz, dWz, Bz, dBz, Kp, tmpX, tmpC, dW1, dW2, dK, ws, ch, Cc):
    """Parameter-gradient epilogue of a level's fused coupling node in one launch (tmg_level_finish): d(kappa) of all NL zero convs
    (fp64 inner products) and the scatter of the grouped weight-gradient rows tmpX / tmpC into dW1 / dW2.  ws: 4 * NL zeroed floats."""
    NL, C = dBz.shape
    for t in (Wz, dWz, Bz, dBz, Kp, tmpX, tmpC, dW1, dW2, dK, ws):
        assert t is None or t.is_contiguous()
    assert ws.numel() >= 4 * NL
    _chk(lib().tmg_level_finish(_ptr(Wz), _ptr(dWz), _ptr(Bz), _ptr(dBz), _ptr(Kp), _ptr(tmpX), _ptr(tmpC), _ptr(dW1), _ptr(dW2), _ptr(dK),
                                _ptr(ws), _i64(NL, C, ch, Cc, tmpC.shape[1] if tmpC is not None else 4), _stream()), "tmg_level_finish")


def adam_step(tab, chunks, nchunks, lr, b1, b2, eps, wd, bc1, bc2s, amsgrad):
    """One launch for the Adam / AMSGrad update of every parameter (tmg_adam_step): tab int64 [n][5] pointers, chunks int32 [nchunks][3]."""
    _chk(lib().tmg_adam_step(_ptr(tab), _ptr(chunks), _i64(nchunks, 1 if amsgrad else 0), _flts([lr, b1, b2, eps, wd, bc1, bc2s, 1.0 - b1, 1.0 - b2]), _stream()),
         "tmg_adam_step")


def mix_f32(x, W, bias, y, transposed=False):
    """y = W x + bias per pixel (W^T when `transposed`: the input gradient of the same mix) in fp32 on the matrix cores, for
    C <= 128 (tmg_mix_f32): the stand-alone 1x1 mixes of the wide levels / ConvLSTM blocks.  False when C is outside the envelope."""
    B, Hh, Ww, C = x.shape
    if C > 128 or C % 4:
        return False
    _chk(lib().tmg_mix_f32(_ptr(x), _d2(x), _ptr(W), _ptr(bias), _ptr(y), _d2(y), _i64(B * Hh * Ww, C, 1 if transposed else 0), _stream()),
         "tmg_mix_f32")
    return True


def mix_affine_fwd(x, hh, W, bias, y, r, y2, logdet):
    """Coupling (generative direction) + trailing mix in one launch (tmg_mix_f32_affine_fwd).  False outside the envelope."""
    B, Hh, Ww, C = x.shape
    rc = lib().tmg_mix_f32_affine_fwd(_ptr(x), _d2(x), _ptr(hh), _d2(hh), _ptr(W), _ptr(bias), _ptr(y), _d2(y), _ptr(r), _ptr(y2),
                                      _ptr(logdet), _i64(B * Hh * Ww, C, Hh * Ww), _stream())
    return _launched(rc, "tmg_mix_f32_affine_fwd")


def mix_affine_bwd(dy, W, r, t2, g, kappa, dto1, dtin2, dhh):
    """Input gradient of the mix + the coupling's backward in one launch (tmg_mix_f32_affine_bwd).  False outside the envelope."""
    B, Hh, Ww, C = dy.shape
    rc = lib().tmg_mix_f32_affine_bwd(_ptr(dy), _d2(dy), _ptr(W), _ptr(r), _ptr(t2), _d2(t2), _ptr(g), _ptr(kappa), _ptr(dto1), _ptr(dtin2),
                                      _d2(dtin2), _ptr(dhh), _d2(dhh), _i64(B * Hh * Ww, C, Hh * Ww), _stream())
    return _launched(rc, "tmg_mix_f32_affine_bwd")


def conv_rep_border_fix(dy, w, outs, kappa=None):
    B, H, W, Cdy = dy.shape
    op, odesc, n_out = _segs(outs)
    Cx = sum(t.shape[3] for t in outs)
    _chk(lib().tmg_conv_rep_border_fix(_ptr(dy), _d2(dy), _ptr(w), _ptr(kappa), op, odesc, c_i64(n_out), _i64(B, H, W, Cdy, Cx),
                                       _stream()), "tmg_conv_rep_border_fix")


# Launch-plan queries (tmg_conv_fwd_plan / tmg_conv_wgrad_plan / tmg_conv_rep_border_plan, tmg_conv_wino_*_plan, tmg_c1x2_fwd_plan / tmg_c1_fwd_plan /
# tmg_conv_wgrad_thin_grouped_plan / tmg_mix_wgrad_grouped_plan): which kernel instance, tiling and grid the
# launcher would use.  Nothing is launched and no pointer is dereferenced, so they run without a device.  An activation is a tensor (as
# in the launching wrappers) or a descriptor ((B, H, W), address, pixel stride, channels) standing for one; an optional operand that
# only has to be present or absent (bias, kappa, in_scale, ws, dbias) may be any true value.
FWD_PLAN_FIELDS = ("kernel", "MT", "NTW", "WM", "WN", "TW_log2", "TH", "tiles_x", "tiles_y", "KCH", "nchunks", "grid_x", "grid_y",
                   "lds_bytes", "vec4", "ovec4")
WGRAD_PLAN_FIELDS = ("NP", "NCO", "LEAN", "ksplit", "MPIX", "TH", "TW_log2", "CITG", "PPG", "gx", "gy", "gz", "slab", "lds_bytes",
                     "ws_floats")
BORDER_PLAN_FIELDS = ("mfma", "NT", "S", "tiles", "blocks")
PLAN_ARGTYPES = {
    "tmg_conv_fwd_plan": [c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp],
    "tmg_conv_wgrad_plan": [c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp],
    "tmg_conv_rep_border_plan": [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp],
    "tmg_conv_wino_fwd_plan": [c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp],
    "tmg_conv_wino_fwd3_plan": [c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp],
    "tmg_conv_wino_narrow_plan": [c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp],
    "tmg_conv_wino_wgrad_plan": [c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp],
    "tmg_c1x2_fwd_plan": [c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp],
    "tmg_c1_fwd_plan": [c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp],
    "tmg_conv_wgrad_thin_grouped_plan": [c_vp, c_i64, c_vp, c_i64, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp],
    "tmg_mix_wgrad_grouped_plan": [c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp],
}
C1X2_PLAN_FIELDS = ("CG", "TW_log2", "TH", "tiles_x", "tiles_y", "t256", "KCH", "nchunks", "nring", "grid", "lds_bytes", "vec4")
C1_PLAN_FIELDS = ("TW_log2", "TH", "tiles_x", "tiles_y", "KCH", "nchunks", "grid", "lds_bytes", "vec4")
THIN_PLAN_FIELDS = ("SL", "CS", "TH", "dyc", "tiles_x", "tiles_y", "ntiles", "P", "xcd", "grid", "lds_bytes")
MIX_WGRAD_PLAN_FIELDS = ("CT", "U", "P", "per", "grid")
WINO_FWD_PLAN_FIELDS = ("kernel", "NPW", "Cin_pad", "nchunks", "last_groups", "ntt", "tiles_x", "tiles_y", "ntiles", "grid_x", "grid_y",
                        "max_tiles", "lds_bytes")
WINO_KERNELS = ("wino_fwd_kernel", "wino_fwdp_kernel", "wino_fwd3_kernel", "wino_nn_kernel")     # plan field "kernel"
WINO_WGRAD_PLAN_FIELDS = ("CIT", "NCO", "DB", "gx", "gy", "gz", "bpg", "NG", "ntiles", "lds_bytes", "ws_floats")


def _pseg(t):
    """(shape[:3], address, pixel stride, channels) of a tensor or of a descriptor of one."""
    if isinstance(t, torch.Tensor):
        B, H, W, C = t.shape
        d = seg(t)
        return (B, H, W), d[0], d[1], d[3]
    shp, addr, stride, n = t
    return tuple(shp), int(addr), int(stride), int(n)


def _psegs(ts):
    d = [_pseg(t) for t in ts]
    return (c_vp * len(d))(*[x[1] for x in d]), (c_i64 * (3 * len(d)))(*[v for x in d for v in (x[2], 0, x[3])]), len(d), d


def _pp(t):
    """Address of an optional operand: a tensor's, a descriptor's, an integer, or 16 for any other true value."""
    if t is None or t is False:
        return c_vp(0)
    if isinstance(t, torch.Tensor):
        return c_vp(t.data_ptr())
    if isinstance(t, tuple):
        return c_vp(int(t[1]))
    return c_vp(16 if t is True else int(t))


def _plan_call(name, fields, *args):
    buf = (c_i64 * len(fields))()
    rc = getattr(lib(), name)(*(args + (buf,)))
    out = dict(zip(fields, [int(v) for v in buf]))
    out["rc"] = int(rc)
    return out


def conv_fwd_plan(inputs, Cout, ksize, stride, outs, bias=None, kappa=None, in_scale=None, in_shift=None, relu_in=False,
                  pad_rep=False, relu_out=False, accumulate=False, add=None):
    """The launch plan of conv_fwd with these arguments: a dict of FWD_PLAN_FIELDS plus "rc", the code the launch would return."""
    ip, idesc, n_in, di = _psegs(inputs)
    op, odesc, n_out, do = _psegs(outs)
    (B, Hin, Win), (_, Hout, Wout) = di[0][0], do[0][0]
    Cin = sum(x[3] for x in di)
    dims = _i64(B, Hin, Win, Hout, Wout, ksize, stride, Cin, Cout, relu_in, pad_rep, relu_out, accumulate)
    ad = _i64(_pseg(add)[2], 0) if add is not None else _i64(0, 0)
    return _plan_call("tmg_conv_fwd_plan", FWD_PLAN_FIELDS, ip, idesc, n_in, c_vp(16), _pp(bias), _pp(kappa), _pp(in_scale),
                      _pp(in_shift), _pp(add), ad, op, odesc, n_out, dims, None)


def conv_wgrad_plan(inputs, dy, ksize, stride, dbias=None, kappa=None, in_scale=None, in_shift=None, relu_in=False, pad_rep=False,
                    use_ws=True, cin_dst=0, cin_valid=0, ci_split=0, ci_off0=0, ci_off1=0, ngroups=1):
    """The launch plan of conv_wgrad's direct kernel (tmg_conv_wgrad; ngroups > 1: of a grouped launch) with these arguments: a dict
    of WGRAD_PLAN_FIELDS plus "rc".  use_ws stands for a workspace of the size the library asks for."""
    ip, idesc, n_in, di = _psegs(inputs)
    (B, Hin, Win) = di[0][0]
    (_, Hout, Wout), dyp, dys, Cout = _pseg(dy)
    Cin = sum(x[3] for x in di)
    dims = _i64(B, Hin, Win, Hout, Wout, ksize, stride, Cin, Cout, relu_in, pad_rep, cin_dst, cin_valid, ci_split, ci_off0, ci_off1)
    need = lib().tmg_conv_wgrad_grouped_ws_floats(dims, c_i64(ngroups)) if ngroups > 1 else lib().tmg_conv_wgrad_ws_floats(dims)
    return _plan_call("tmg_conv_wgrad_plan", WGRAD_PLAN_FIELDS, ip, idesc, n_in, _pp(in_scale), _pp(in_shift), c_vp(dyp), _i64(dys, 0),
                      c_vp(16), _pp(dbias), _pp(kappa), c_vp(16 if use_ws else 0), c_i64(need if use_ws else 0), dims, None, c_i64(ngroups))


def conv_rep_border_plan(dy, outs):
    """The launch plan of conv_rep_border_fix(dy, w, outs): a dict of BORDER_PLAN_FIELDS plus "rc"."""
    (B, H, W), dyp, dys, Cdy = _pseg(dy)
    op, odesc, n_out, do = _psegs(outs)
    Cx = sum(x[3] for x in do)
    return _plan_call("tmg_conv_rep_border_plan", BORDER_PLAN_FIELDS, c_vp(dyp), _i64(dys, 0), c_vp(16), c_vp(0), op, odesc, n_out,
                      _i64(B, H, W, Cdy, Cx), None)


def _wino_fwd_plan(name, inputs, Cout, outs, bias, *flags):
    ip, idesc, n_in, di = _psegs(inputs)
    op, odesc, n_out, do = _psegs(outs)
    (B, Hin, Win) = di[0][0]
    Cin = sum(x[3] for x in di)
    return _plan_call(name, WINO_FWD_PLAN_FIELDS, ip, idesc, n_in, c_vp(16), _pp(bias), op, odesc, n_out,
                      _i64(B, Hin, Win, Cin, Cout, *flags), None)


def conv_wino_fwd_plan(inputs, Cout, outs, bias=None, relu_in=False, pad_rep=False):
    """The launch plan of conv_wino_fwd with these arguments: a dict of WINO_FWD_PLAN_FIELDS plus "rc", the code the launch would return
    (-100: outside the envelope, conv_wino_fwd returns False)."""
    return _wino_fwd_plan("tmg_conv_wino_fwd_plan", inputs, Cout, outs, bias, relu_in, pad_rep)


def conv_wino_fwd3_plan(inputs, Cout, outs, bias=None, relu_in=False, pad_rep=False):
    """The launch plan of conv_wino_fwd3 (as conv_wino_fwd_plan)."""
    return _wino_fwd_plan("tmg_conv_wino_fwd3_plan", inputs, Cout, outs, bias, relu_in, pad_rep)


def conv_wino_narrow_plan(inputs, Cout, outs, bias=None, relu_in=False, pad_rep=False, relu_out=False):
    """The launch plan of conv_wino_narrow (as conv_wino_fwd_plan; "NPW" holds NTN)."""
    return _wino_fwd_plan("tmg_conv_wino_narrow_plan", inputs, Cout, outs, bias, relu_in, pad_rep, relu_out)


def conv_wino_wgrad_plan(inputs, dy, dbias=None, relu_in=False, pad_rep=False, cin_dst=0, cin_valid=0, ci_split=0, ci_off0=0, ci_off1=0,
                         ngroups=1, use_ws=True):
    """The launch plan of conv_wino_wgrad (ngroups > 1: of conv_wgrad_grouped's Winograd launch of that many groups, dy standing for ONE
    group's channels) with these arguments: a dict of WINO_WGRAD_PLAN_FIELDS plus "rc".  use_ws stands for a workspace of the size the
    library asks for."""
    ip, idesc, n_in, di = _psegs(inputs)
    (B, Hin, Win) = di[0][0]
    _, dyp, dys, Cout = _pseg(dy)
    Cin = sum(x[3] for x in di)
    wd = _i64(B, Hin, Win, Cin, Cout, relu_in, pad_rep, cin_dst, cin_valid, ci_split, ci_off0, ci_off1)
    need = lib().tmg_conv_wino_wgrad_grouped_ws_floats(wd, c_i64(ngroups)) if ngroups > 1 else lib().tmg_conv_wino_wgrad_ws_floats(wd)
    return _plan_call("tmg_conv_wino_wgrad_plan", WINO_WGRAD_PLAN_FIELDS, ip, idesc, n_in, c_vp(dyp), _i64(dys, 0), c_vp(16), _pp(dbias),
                      c_vp(16 if use_ws else 0), c_i64(need if use_ws else 0), wd, None, c_i64(ngroups))


def c1x2_fwd_plan(inputs, out, add1=None, add2=None, w_rows=0, w2_d1_row=0, w_split=0, w_gap=0, relu_in=True):
    """The launch plan of c1x2_fwd with these arguments: a dict of C1X2_PLAN_FIELDS plus "rc"."""
    ip, idesc, n_in, di = _psegs(inputs)
    (B, Hh, Ww) = di[0][0]
    Cin = sum(x[3] for x in di)
    _, op, ostr, _ = _pseg(out)
    d2 = lambda t: _i64(_pseg(t)[2], 0) if t is not None else _i64(0, 0)      # noqa: E731
    return _plan_call("tmg_c1x2_fwd_plan", C1X2_PLAN_FIELDS, ip, idesc, n_in, c_vp(16), c_vp(16), _pp(add1), d2(add1), _pp(add2), d2(add2),
                      c_vp(op), _i64(ostr, 0), _i64(B, Hh, Ww, Cin, relu_in, w_rows, w_split, w_gap, w2_d1_row), None)


def c1_fwd_plan(inputs, out, add=None, w_rows=0, fill4=False, w_split=0, w_gap=0, relu_in=True):
    """The launch plan of c1_fwd with these arguments: a dict of C1_PLAN_FIELDS plus "rc"."""
    ip, idesc, n_in, di = _psegs(inputs)
    (B, Hh, Ww) = di[0][0]
    Cin = sum(x[3] for x in di)
    _, op, ostr, _ = _pseg(out)
    ad = _i64(_pseg(add)[2], 0) if add is not None else _i64(0, 0)
    return _plan_call("tmg_c1_fwd_plan", C1_PLAN_FIELDS, ip, idesc, n_in, c_vp(16), _pp(add), ad, c_vp(op), _i64(ostr, 0),
                      _i64(B, Hh, Ww, Cin, relu_in, w_rows, fill4, w_split, w_gap), None)


def conv_wgrad_thin_grouped_plan(shape3, seg_channels, G, dy_addr, dy_stride, dyc, relu_in=True):
    """The launch plan of conv_wgrad_thin_grouped: G groups of inputs [B, H, W, sum(seg_channels)] (shape3 = (B, H, W)), the shared
    dy at address dy_addr with pixel stride dy_stride and dyc channels per group: a dict of THIN_PLAN_FIELDS plus "rc" (-100: declined)."""
    B, Hh, Ww = shape3
    return _plan_call("tmg_conv_wgrad_thin_grouped_plan", THIN_PLAN_FIELDS, c_vp(16), c_i64(G), _i64(*seg_channels), c_i64(len(seg_channels)),
                      c_vp(int(dy_addr)), c_i64(dy_stride), c_vp(16), _i64(B, Hh, Ww, sum(seg_channels), relu_in, dyc), None)


def mix_wgrad_grouped_plan(npix, C, G, db=True):
    """The launch plan of mix_wgrad_grouped for G groups of npix pixels and C channels: a dict of MIX_WGRAD_PLAN_FIELDS plus "rc"."""
    return _plan_call("tmg_mix_wgrad_grouped_plan", MIX_WGRAD_PLAN_FIELDS, c_vp(16), c_i64(G), c_vp(16), _pp(db), _i64(npix, C), None)


def conv_dgrad_direct(dy, w, dx, ksize, stride, accumulate=False):
    B, Hin, Win, Cin = dx.shape
    _, Hout, Wout, Cout = dy.shape
    _chk(lib().tmg_conv_dgrad_direct(_ptr(dy), _d2(dy), _ptr(w), _ptr(dx), _d2(dx),
                                     _i64(B, Hin, Win, Hout, Wout, Cin, Cout, ksize, stride, accumulate), _stream()),
         "tmg_conv_dgrad_direct")


# ------------------------------------------------------------------------------------------------
# bandwidth-bound ops
# ------------------------------------------------------------------------------------------------
def affine_apply(hh, x2, y2, rsave, logdet, reverse, x1=None, y1=None):
    """x1 / y1 (optional, Ch channels each): pass-through half copied in the same launch."""
    B, H, W, Ch = x2.shape
    if x1 is None:
        _chk(lib().tmg_affine_apply(_ptr(hh), _d2(hh), _ptr(x2), _d2(x2), _ptr(y2), _d2(y2), _ptr(rsave), _ptr(logdet),
                                    _i64(B, H * W, Ch, reverse), _stream()), "tmg_affine_apply")
    else:
        assert x1.shape == x2.shape and y1.shape == x2.shape
        _chk(lib().tmg_affine_apply_pass(_ptr(hh), _d2(hh), _ptr(x2), _d2(x2), _ptr(y2), _d2(y2), _ptr(rsave), _ptr(logdet), _ptr(x1),
                                         _d2(x1), _ptr(y1), _d2(y1), _i64(B, H * W, Ch, reverse), _stream()), "tmg_affine_apply_pass")


def affine_bwd(gout, yref, rsave, g, gin, dhh, reverse, kappa=None):
    """kappa given: dhh is written pre-multiplied by exp(clamp(kappa))."""
    B, H, W, Ch = gout.shape
    _chk(lib().tmg_affine_bwd_scaled(_ptr(gout), _d2(gout), _ptr(yref), _d2(yref), _ptr(rsave), _ptr(g), _ptr(gin), _d2(gin), _ptr(dhh),
                                     _d2(dhh), _ptr(kappa), _i64(B, H * W, Ch, reverse), _stream()), "tmg_affine_bwd_scaled")


def lstm_pointwise_fwd(gates, c_prev, c_next, h_next):
    B, H, W, R4 = gates.shape
    _chk(lib().tmg_lstm_pointwise_fwd(_ptr(gates), _ptr(c_prev), _d2(c_prev), _ptr(c_next), _ptr(h_next), _i64(B * H * W, R4 // 4), _stream()),
         "tmg_lstm_pointwise_fwd")


def lstm_pointwise_bwd(acts, c_prev, c_next, dh, dc_in, dc_prev):
    B, H, W, R4 = acts.shape
    _chk(lib().tmg_lstm_pointwise_bwd(_ptr(acts), _ptr(c_prev), _d2(c_prev), _ptr(c_next), _ptr(dh), _ptr(dc_in), _ptr(dc_prev),
                                      _i64(B * H * W, R4 // 4), _stream()), "tmg_lstm_pointwise_bwd")


def gauss_fwd(hz, zin, zout, logp, mode, clip_mean, limits):
    B, H, W, Ch = zin.shape
    _chk(lib().tmg_gauss_fwd(_ptr(hz), _d2(hz), _ptr(zin), _d2(zin), _ptr(zout), _d2(zout), _ptr(logp), _i64(B, H * W, Ch, mode, clip_mean),
                             _flts(limits), _stream()), "tmg_gauss_fwd")


def gauss_bwd(hz, zin, dzin, g, dzout, dhz, mode, clip_mean, limits):
    B, H, W, Ch = zin.shape
    _chk(lib().tmg_gauss_bwd(_ptr(hz), _d2(hz), _ptr(zin), _d2(zin), _ptr(dzin), _d2(dzin), _ptr(g), _ptr(dzout), _d2(dzout), _ptr(dhz), _d2(dhz),
                             _i64(B, H * W, Ch, mode, clip_mean), _flts(limits), _stream()), "tmg_gauss_bwd")


def gauss_sample(hz, eps, z1, out, logp, clip_mean, limits, eps_out=None, nonce=None, site=0):
    """out[..., C - Ch:] = mean + exp(log-std) eps, out[..., :Ch] = z1 (when given): the Gaussian sample written straight into the
    level's activation (tmg_gauss_sample).  eps None: drawn in the kernel from (nonce, site) and stored to eps_out."""
    B, Hh, Ww, Co = out.shape
    Ch = hz.shape[3] // 2
    off = Co - Ch
    od = seg(out)
    _chk(lib().tmg_gauss_sample(_ptr(hz), _d2(hz), _ptr(eps), _d2(eps), _ptr(z1), _d2(z1), _ptr(out), _i64(od[1], off), c_i64(0), _ptr(eps_out),
                                _ptr(logp), _ptr(nonce), _i64(B, Hh * Ww, Ch, clip_mean, site), _flts(limits), _stream()), "tmg_gauss_sample")


def gauss_sample_keyed(hz, eps, z1, out, logp, clip_mean, limits, keys, rows_per_key, site=0, eps_out=None):
    """gauss_sample for a batch of members of rows_per_key images each: member m draws with key row m of `keys` ([K, 2] int64 on the
    device) exactly the latents a rows_per_key-image gauss_sample call keyed by that row draws (tmg_gauss_sample_keyed)."""
    B, Hh, Ww, Co = out.shape
    Ch = hz.shape[3] // 2
    off = Co - Ch
    od = seg(out)
    if eps is None and (keys is None or keys.dtype != torch.int64 or not keys.is_cuda or not keys.is_contiguous()
                        or keys.numel() != 2 * (B // max(int(rows_per_key), 1))):
        raise RuntimeError("gauss_sample_keyed needs a contiguous [B / rows_per_key, 2] int64 key table on the device")
    _chk(lib().tmg_gauss_sample_keyed(_ptr(hz), _d2(hz), _ptr(eps), _d2(eps), _ptr(z1), _d2(z1), _ptr(out), _i64(od[1], off), c_i64(0),
                                      _ptr(eps_out), _ptr(logp), _ptr(keys), _i64(B, Hh * Ww, Ch, clip_mean, site, rows_per_key),
                                      _flts(limits), _stream()), "tmg_gauss_sample_keyed")


def ens_accum(y, u, out_mu, out_std, smean, sm2, tmean, tm2, outs, ostrides, k, n_before, m0, t_before, flags):
    """Fold one roll-out step of k members (y: NHWC [k*B, H, W, C] or a channel-slice view) into the step's running statistics and,
    flags & 1, the members' time statistics; flags & 2: the step's last chunk, write (mean, std, mag_mean, mag_std) = `outs` with the
    per-case strides ostrides = (channel outputs, magnitude outputs) instead of the step state (tmg_ens_accum)."""
    kB, Hh, Ww, Cc = y.shape
    ptr, ps, co, _ = seg(y)
    outs = outs if outs is not None else (None,) * 4
    _chk(lib().tmg_ens_accum(c_vp(ptr), _i64(ps, co), _ptr(u), _ptr(out_mu), _ptr(out_std), _ptr(smean), _ptr(sm2), _ptr(tmean),
                             _ptr(tm2), *[_ptr(t) for t in outs], _i64(*ostrides), _i64(k, kB // k, Hh * Ww, Cc, n_before, m0, t_before, flags),
                             _stream()), "tmg_ens_accum")


def ens_time_finalize(tmean, tm2, tm_mean, tm_std, rms_mean, rms_std, S, B, HW, C, T):
    """Per member time mean and RMS fluctuation over T steps, then their mean / std over the S members (tmg_ens_time_finalize)."""
    _chk(lib().tmg_ens_time_finalize(_ptr(tmean), _ptr(tm2), _ptr(tm_mean), _ptr(tm_std), _ptr(rms_mean), _ptr(rms_std),
                                     _i64(S, B, HW, C, T), _stream()), "tmg_ens_time_finalize")


def ens_turb_accum(y, u, out_mu, out_std, tmean, vmean, vm2, cuv, tvort, outs, ostride, grid, k, n_before, m0, t_before, flags):
    """The turbulence statistics of the chunk ens_accum folds (same y, u, k, n_before, m0, t_before, flags): vorticity on the grid
    (dx, dy) into the step state (vmean, vm2) or, flags & 2, as (vort_mean, vort_std) = `outs` with per-case stride ostride; flags & 1
    advances the members' time co-moment cuv and time-mean vorticity tvort.  Reads the time means ens_accum keeps in tmean as they
    stand after t_before steps: call it before ens_accum on the chunk (tmg_ens_turb_accum)."""
    kB, Hh, Ww, Cc = y.shape
    ptr, ps, co, _ = seg(y)
    outs = outs if outs is not None else (None,) * 2
    _chk(lib().tmg_ens_turb_accum(c_vp(ptr), _i64(ps, co), _ptr(u), _ptr(out_mu), _ptr(out_std), _ptr(tmean), _ptr(vmean), _ptr(vm2),
                                  _ptr(cuv), _ptr(tvort), *[_ptr(t) for t in outs],
                                  _i64(k, kB // k, Hh, Ww, Cc, n_before, m0, t_before, flags, ostride), _flts(grid), _stream()),
         "tmg_ens_turb_accum")


def ens_turb_finalize(tm2, cuv, tvort, outs, S, B, HW, C, T):
    """Per member <u'v'>, 0.5 (<u'u'> + <v'v'>) and time-mean vorticity over T steps, then mean / std of each over the S members into
    outs = (uv_mean, uv_std, tke_mean, tke_std, vort_mean, vort_std) (tmg_ens_turb_finalize)."""
    _chk(lib().tmg_ens_turb_finalize(_ptr(tm2), _ptr(cuv), _ptr(tvort), *[_ptr(t) for t in outs], _i64(S, B, HW, C, T), _stream()),
         "tmg_ens_turb_finalize")


def ens_score_store(y, xs, k, m0):
    """Copy one chunk of k members (y: NHWC [k*B, H, W, C] or a channel-slice view, rows member-major) into rows m0 .. m0 + k - 1 of
    the planar member buffer xs [S, B, C, HW], values unchanged (tmg_ens_score_store)."""
    kB, Hh, Ww, Cc = y.shape
    ptr, ps, co, _ = seg(y)
    _chk(lib().tmg_ens_score_store(c_vp(ptr), _i64(ps, co), _ptr(xs), _i64(k, kB // k, Hh * Ww, Cc, xs.shape[0], m0), _stream()),
         "tmg_ens_score_store")


def ens_score_step(xs, target, scale, crps, crps_fair, hist, tmeans, ostrides, t_before, flags):
    """Score one kept step whose S members are in xs [S, B, C, HW] against target (NHWC [B, H, W, C] or a channel-slice view): CRPS and
    fair CRPS times scale [B, C] into crps / crps_fair, the targets' ranks into the int32 histogram hist, with the per-case strides
    ostrides = (scores, histogram); flags & 1 advances the running time means tmeans = (tcrps, tcrps_fair) that hold t_before steps
    (tmg_ens_score_step)."""
    S, B, Cc, HW = xs.shape
    ptr, ps, co, _ = seg(target)
    tmeans = tmeans if tmeans is not None else (None,) * 2
    _chk(lib().tmg_ens_score_step(_ptr(xs), c_vp(ptr), _i64(ps, co), _ptr(scale), _ptr(crps), _ptr(crps_fair), _ptr(hist),
                                  *[_ptr(t) for t in tmeans], _i64(*ostrides), _i64(S, B, HW, Cc, t_before, flags), _stream()),
         "tmg_ens_score_step")


def ens_quant_step(xs, target, u, out_mu, out_std, lo, hi, w, thr, ex, quant, exceed, taggs, ostrides, t_before, flags):
    """Order statistics of one kept step whose S members are in xs [S, B, C, HW]: the Q levels (lo, hi, w) (host sequences: ranks
    and the fp32 weight between them) un-normalised by u [B, C] or None, out_mu, out_std into quant; the K thresholds ex = ((channel,
    1 for > / 0 for <), ..) with the raw values thr [B, K] (device) as exceedance probabilities into exceed; per-case strides ostrides
    = (quant, exceed).  flags & 1 advances the time aggregates taggs = (tquant, tbelow int32, texceed int32) that hold t_before steps;
    flags & 2: target (NHWC [B, H, W, C] or a channel-slice view) is given and tbelow counts the steps with target < quantile
    (tmg_ens_quant_step)."""
    S, B, Cc, HW = xs.shape
    ptr, ps, co, _ = seg(target) if target is not None else (0, 0, 0, 0)
    taggs = taggs if taggs is not None else (None,) * 3
    lohi = [int(v) for pair in zip(lo, hi) for v in pair]
    exf = [int(v) for e in ex for v in e]
    _chk(lib().tmg_ens_quant_step(_ptr(xs), c_vp(ptr), _i64(ps, co), _ptr(u), _ptr(out_mu), _ptr(out_std), _i64(*lohi),
                                  _flts([float(v) for v in w]), _ptr(thr), _i64(*exf) if exf else None, _ptr(quant), _ptr(exceed),
                                  *[_ptr(t) for t in taggs], _i64(*ostrides), _i64(S, B, HW, Cc, len(lohi) // 2, len(exf) // 2, t_before, flags),
                                  _stream()), "tmg_ens_quant_step")


def ens_gram_plan(S, B, C, HW):
    """The launch plan of ens_gram_step for S members of [B, C, HW] (tmg_ens_gram_plan; nothing is launched) -> dict: P pixel slices of
    SL pixels, L the fmaf terms of one partial (L P >= HW), NT row macro-tiles of 64 rows over the S + 1 rows, pairs = the NT (NT + 1) / 2
    macro-tile pairs (I, J), I <= J, in workspace order, part the floats of one partial, ws the workspace floats."""
    plan = (c_i64 * 7)()
    _chk(lib().tmg_ens_gram_plan(_i64(S, B, C, HW), plan), "tmg_ens_gram_plan")
    P, L, NP, ws, SL, NT, part = [int(v) for v in plan]
    pairs = [(i, j) for i in range(NT) for j in range(i, NT)]
    assert len(pairs) == NP
    return {"P": P, "L": L, "pairs": pairs, "ws": ws, "SL": SL, "NT": NT, "part": part}


def ens_gram_step(xs, target, a2, groups, r, ws, traj, outf, outi, t, t_before, flags):
    """Energy score and member distances of one kept step whose S members are in xs [S, B, C, HW], against target (NHWC [B, H, W, C] or
    a channel-slice view) as row S: the members' mean into r [B, C, HW], the Gram partials into the workspace ws (>= ens_gram_plan's
    floats), then per case and channel group (groups: tuples of channels; a2 [B, C]: the squared scales) the step's scores into
    outf [5, B, Tk, Gn] / outi [2, B, Tk, Gn] int64 at step t; flags & 1 adds the squared distances to traj [B, Gn, S + 1, S + 1],
    which holds t_before steps (tmg_ens_gram_step)."""
    S, B, Cc, HW = xs.shape
    ptr, ps, co, _ = seg(target)
    grp = [-1] * 16
    for g, chs in enumerate(groups):
        for k, ch in enumerate(chs):
            grp[4 * g + k] = int(ch)
    _chk(lib().tmg_ens_gram_step(_ptr(xs), c_vp(ptr), _i64(ps, co), _ptr(a2), _i64(*grp), _ptr(r), _ptr(ws), c_i64(ws.numel()),
                                 _ptr(traj), _ptr(outf), _ptr(outi), _i64(S, B, HW, Cc, len(groups), outf.shape[2], t, t_before, flags),
                                 _stream()), "tmg_ens_gram_step")


def ens_gram_traj(traj, outf, outi):
    """The scores and argmins of ens_gram_step on sqrt(traj), traj [B, Gn, S + 1, S + 1], into outf [5, B, Gn] / outi [2, B, Gn] int64
    (tmg_ens_gram_traj)."""
    B, Gn, R, _ = traj.shape
    _chk(lib().tmg_ens_gram_traj(_ptr(traj), _ptr(outf), _ptr(outi), _i64(R - 1, B, Gn), _stream()), "tmg_ens_gram_traj")


def ens_sfun_plan(S, B, C, H, W, lags):
    """The launch plan of ens_sfun_step for S members of [B, C, H, W] and the lags [(dx, dy), ..] (tmg_ens_sfun_plan; nothing is
    launched) -> dict: P pixel slices of SL pixels (pixel i W + j), threads = 256 (thread t walks the pixels t, t + 256, .. of its
    slice), Lc the fp32 additions along the longest path inside one partial, R = S + 1 rows, ws the workspace floats, and per lag
    off / jmax / ilo / ihi / N: the pair (p, p + off) is counted at pixel p when j < jmax and ilo <= i < ihi, N of them."""
    lags = [(int(dx), int(dy)) for dx, dy in lags]
    L = len(lags)
    plan = (c_i64 * 88)()
    _chk(lib().tmg_ens_sfun_plan(_i64(S, B, C, H, W, L), _i64(*[v for l in lags for v in l]) if L else None, plan), "tmg_ens_sfun_plan")
    P, Lc, ws, SL, threads, Lq, R = [int(v) for v in plan[:7]]
    assert Lq == L
    per = [[int(v) for v in plan[8 + 5 * l:13 + 5 * l]] for l in range(L)]
    return {"P": P, "Lc": Lc, "ws": ws, "SL": SL, "threads": threads, "L": L, "R": R, "lags": lags,
            "off": [q[0] for q in per], "jmax": [q[1] for q in per], "ilo": [q[2] for q in per], "ihi": [q[3] for q in per],
            "N": [q[4] for q in per]}


def ens_sfun_step(xs, target, lags, ws, mom, vsum, tmom, tvar, H, W, t_before, flags):
    """Raw structure-function and variogram sums of one kept step whose S members are in xs [S, B, C, H W], against target (NHWC
    [B, H, W, C] or a channel-slice view) as row S, at the lags [(dx, dy), ..]: mom [3, B, C, L, S + 1] (the sums of the increments'
    squares, cubes and fourth powers), vsum [B, C, L]; flags & 1 adds them to tmom / tvar, which hold t_before steps; ws: the
    workspace (>= ens_sfun_plan's floats) (tmg_ens_sfun_step)."""
    S, B, Cc, HW = xs.shape
    ptr, ps, co, _ = seg(target)
    _chk(lib().tmg_ens_sfun_step(_ptr(xs), c_vp(ptr), _i64(ps, co), _i64(*[int(v) for l in lags for v in l]), _ptr(ws), c_i64(ws.numel()),
                                 _ptr(mom), _ptr(vsum), _ptr(tmom), _ptr(tvar), _i64(S, B, Cc, H, W, len(lags), t_before, flags),
                                 _stream()), "tmg_ens_sfun_step")


EVENT_PLAN_FIELDS = ("TH", "TW", "halo", "NTY", "NTX", "lds", "threads", "ws", "pitch", "rows", "blocks")


def ens_event_plan(S, B, H, W, K, scales):
    """The launch plan of ens_event_step's neighbourhood kernel for S members of B cases of [H, W], K events and the odd widths
    `scales` (tmg_ens_event_plan; nothing is launched) -> dict: one block per TH x TW tile of one (case, event) plane, NTY x NTX tiles,
    halo = the largest w // 2 (the block loads its tile plus that many pixels on every side, zeros outside the field), two LDS
    tables of `rows` rows of `pitch` ints (summed-area tables with a zero row and column), lds bytes per block, threads, ws = 0
    workspace, blocks = NTY NTX K B."""
    scales = [int(w) for w in scales]
    plan = (c_i64 * 12)()
    _chk(lib().tmg_ens_event_plan(_i64(S, B, H, W, K, len(scales)), _i64(*scales) if scales else None, plan), "tmg_ens_event_plan")
    out = {k: int(v) for k, v in zip(EVENT_PLAN_FIELDS, plan)}
    out["scales"] = scales
    return out


def ens_event_count(y, thr, ev, cnt, S, k, m0):
    """Count one chunk of k members (y: NHWC [k*B, H, W, C] or a channel-slice view, rows member-major) against the K events ev =
    ((channel, 1 for > / 0 for <), ..) with the raw thresholds thr [B, K] (device) into cnt [B, K, HW] int32: m0 = 0 writes, later
    chunks add (tmg_ens_event_count)."""
    kB, Hh, Ww, Cc = y.shape
    ptr, ps, co, _ = seg(y)
    evf = [int(v) for e in ev for v in e]
    _chk(lib().tmg_ens_event_count(c_vp(ptr), _i64(ps, co), _ptr(thr), _i64(*evf) if evf else None, _ptr(cnt),
                                   _i64(k, kB // k, Hh * Ww, Cc, S, m0, len(ev)), _stream()), "tmg_ens_event_count")


def ens_event_step(cnt, target, thr, ev, scales, rel_count, rel_hit, fss_raw, tsum, ostrides, S, t_before, flags):
    """Verify one kept step whose member counts are in cnt [B, K, HW] int32 against target (NHWC [B, H, W, C] or a channel-slice
    view): the reliability tables into rel_count / rel_hit (int32, [K, S + 1] per case) and the raw fractions-skill sums (A, Bx, Cc)
    per width of `scales` into fss_raw (int64, [K, NS, 3] per case), with the per-case strides ostrides = (tables, raw sums); the
    step's planes are zeroed first.  flags & 1 advances the per-pixel sums tsum [4, B, K, HW] int32 (n, o, n^2, n o) that hold
    t_before steps (tmg_ens_event_step)."""
    B, Hh, Ww, Cc = target.shape
    ptr, ps, co, _ = seg(target)
    evf = [int(v) for e in ev for v in e]
    scales = [int(w) for w in scales]
    _chk(lib().tmg_ens_event_step(_ptr(cnt), c_vp(ptr), _i64(ps, co), _ptr(thr), _i64(*evf) if evf else None,
                                  _i64(*scales) if scales else None, _ptr(rel_count), _ptr(rel_hit), _ptr(fss_raw), _ptr(tsum),
                                  _i64(*ostrides), _i64(S, B, Hh, Ww, Cc, len(ev), len(scales), t_before, flags), _stream()),
         "tmg_ens_event_step")


PDF_PLAN_FIELDS = ("SL", "NSL", "lds", "copies", "instance", "threads", "blocks", "PPT")
PDF_KINDS = {"speed": 4, "vort": 5, "div": 6}


def ens_pdf_plan(k, B, H, W, F, nb, P, nbj, R, derived):
    """The launch plan of ens_pdf_count for a chunk of k members of B cases of [H, W], F fields of nb inner bins, P pairs of nbj bins
    per axis, R regions; derived: a field is speed, vort or div (tmg_ens_pdf_plan; nothing is launched) -> dict: one block per slice
    of SL = 256 PPT pixels of one row (member, case), NSL slices per row, lds bytes per block, copies = the private marginal
    histograms, instance (0: channel fields only, 1: with derived fields), threads, blocks = NSL k B."""
    plan = (c_i64 * 8)()
    _chk(lib().tmg_ens_pdf_plan(_i64(k, B, H, W, F, nb, P, nbj, R, 1 if derived else 0), plan), "tmg_ens_pdf_plan")
    return {key: int(v) for key, v in zip(PDF_PLAN_FIELDS, plan)}


def ens_pdf_count(y, u, out_mu, out_std, center, edges, jedges, kinds, pairs, boxes, step_count, step_joint, mtime, tjoint, ostrides, grid,
                  S, k, m0, nb, nbj, flags):
    """Bin one chunk of k members (y: NHWC [k*B, H, W, C] or a channel-slice view, rows member-major) of the fields `kinds` (0..C-1: a
    channel, 4 / 5 / 6: speed / vort / div on grid = (dx, dy)) against the edge tables edges [B, F, nb + 1] / jedges [B, P, 2, nbj + 1]
    (device fp32) over the pixel boxes (x0, x1, y0, y1), the pairs (fi, fj) jointly; center: c_raw [B, C, HW] or None.  Adds into the
    int32 planes step_count ([R, F, nb + 2] per case) / step_joint ([R, P, (nbj + 2)^2] per case) with the per-case strides ostrides,
    and with flags & 1 into mtime [B, S, R, F, nb + 2] (members m0 .. m0 + k - 1) / tjoint [B, R, P, (nbj + 2)^2]
    (tmg_ens_pdf_count)."""
    kB, Hh, Ww, Cc = y.shape
    ptr, ps, co, _ = seg(y)
    desc = [int(v) for v in kinds] + [int(v) for pr in pairs for v in pr] + [int(v) for bx in boxes for v in bx]
    _chk(lib().tmg_ens_pdf_count(c_vp(ptr), _i64(ps, co), _ptr(u), _ptr(out_mu), _ptr(out_std), _ptr(center), _ptr(edges), _ptr(jedges),
                                 _i64(*desc), _ptr(step_count), _ptr(step_joint), _ptr(mtime), _ptr(tjoint), _i64(*ostrides),
                                 _i64(k, kB // k, Hh, Ww, Cc, S, m0, len(kinds), nb, len(pairs), nbj, len(boxes), flags),
                                 _flts(grid) if grid is not None else None, _stream()), "tmg_ens_pdf_count")


def ens_pod_plan(S, B, Cg, HW, K):
    """The slice plan of ens_pod_project for calls of S members of B cases of [Cg, HW] against K modes (tmg_ens_pod_plan; nothing is
    launched) -> dict: P pixel slices of SL pixels (a function of HW alone: the same for every S), L = SL Cg the fmaf terms of one
    partial (L P >= HW Cg), ws the workspace floats of a call of S members (0 for P = 1)."""
    plan = (c_i64 * 4)()
    _chk(lib().tmg_ens_pod_plan(_i64(S, B, Cg, HW, K), plan), "tmg_ens_pod_plan")
    P, SL, L, ws = [int(v) for v in plan]
    return {"P": P, "SL": SL, "L": L, "ws": ws}


def ens_pod_project(y, channels, a, m, psi, ws, coef, en, ostrides, k):
    """Project one chunk of k members (y: NHWC [k*B, H, W, C] or a channel-slice view, rows member-major; k = 1: the B target rows) on
    the modes psi [B, K, Cg, HW] about the mean planes m [B, Cg, HW] with the scales a [B, Cg] (device fp32) over the channels
    `channels`: the raw sums coef_raw [K] and en_raw of row (s, b) at coef + b ostrides[0] + s ostrides[1] and en + b ostrides[2] +
    s ostrides[3] (coef / en: views that start at the chunk's first member and step); ws: the workspace (>= ens_pod_plan's floats
    for S = k) or None when the plan needs none (tmg_ens_pod_project)."""
    kB, Hh, Ww, Cc = y.shape
    ptr, ps, co, _ = seg(y)
    B, K, Cg, HW = psi.shape
    _chk(lib().tmg_ens_pod_project(c_vp(ptr), _i64(ps, co), _i64(*[int(c) for c in channels]), _ptr(a), _ptr(m), _ptr(psi), _ptr(ws),
                                   c_i64(ws.numel() if ws is not None else 0), _ptr(coef), _ptr(en), _i64(*ostrides),
                                   _i64(k, kB // k, Hh * Ww, Cg, K), _stream()), "tmg_ens_pod_project")


def ens_phase_plan(S, B, C, HW, NB):
    """The launch plan of ens_phase_accum for calls of S members of B cases of [C, HW] into NB sectors (tmg_ens_phase_plan; nothing
    is launched) -> dict: tile pixels per block, tiles per field (the grid is tiles x NB x B), ws = 0 workspace floats, vec: True
    when dense 16-byte aligned rows take the vector path (HW % 4 == 0); channel-slice or unaligned rows always take the scalar one."""
    plan = (c_i64 * 6)()
    _chk(lib().tmg_ens_phase_plan(_i64(S, B, C, HW, NB), plan), "tmg_ens_phase_plan")
    tile, tiles, gy, gz, ws, vec = [int(v) for v in plan]
    return {"tile": tile, "tiles": tiles, "grid": (tiles, gy, gz), "ws": ws, "vec": bool(vec)}


def _phase_span(t, strides, k, B, extra, what):
    """A view t addressed at t + b strides[0] + s strides[1] + extra (b < B, s < k) must stay inside its storage."""
    last = t.storage_offset() + (B - 1) * int(strides[0]) + (k - 1) * int(strides[1]) + int(extra)
    if min(int(strides[0]), int(strides[1]), int(extra)) < 0 or last >= t.untyped_storage().nbytes() // t.element_size():
        raise RuntimeError("%s: strides %s reach beyond the tensor for %d x %d rows" % (what, tuple(strides), k, B))


def ens_phase_label(coef, cstrides, pair, g, tab, lab, lstrides, k, B, NB):
    """Label k B rows with the sector of their phase (tmg_ens_phase_label).  coef: a view of the raw coefficient sums that starts at
    the chunk's first member and step, row (s, b) at coef + b cstrides[0] + s cstrides[1], the pair's modes at + pair[0], + pair[1];
    g [B, 2] device fp32; tab: 8 host floats (the gate, then the NB / 4 - 1 tangents); lab: an int32 view, row (s, b) at
    lab + b lstrides[0] + s lstrides[1]."""
    check_act(coef)
    check_act(g)
    if not (lab.is_cuda and lab.dtype == torch.int32):
        raise RuntimeError("the labels are int32 on a HIP device (got %s on %s)" % (lab.dtype, lab.device))
    if tuple(g.shape) != (B, 2) or not g.is_contiguous() or len(tab) != 8:
        raise RuntimeError("ens_phase_label: g is a contiguous [%d, 2] table and tab holds 8 floats" % B)
    _phase_span(coef, cstrides, k, B, max(pair), "ens_phase_label: coef")
    _phase_span(lab, lstrides, k, B, 0, "ens_phase_label: lab")
    _chk(lib().tmg_ens_phase_label(_ptr(coef), _i64(*cstrides), _i64(*pair), _ptr(g), _flts(tab), _ptr(lab), _i64(*lstrides),
                                   _i64(k, B, NB), _stream()), "tmg_ens_phase_label")


def ens_phase_accum(y, lab, lstrides, a, m, acc, k):
    """Add one chunk of k members (y: NHWC [k*B, H, W, C] or a channel-slice view, rows member-major; k = 1: the B target rows) to
    the accumulators acc [B, NB, 2 C + 1, HW] of the sectors their labels name (lab / lstrides as ens_phase_label wrote them), about
    the mean planes m [B, C, HW] with the scales a [B, C] (device fp32) (tmg_ens_phase_accum)."""
    kB, Hh, Ww, Cc = y.shape
    ptr, ps, co, _ = seg(y)
    B, NB, Q, HW = acc.shape
    if Q != 2 * Cc + 1 or HW != Hh * Ww or kB != k * B or tuple(m.shape) != (B, Cc, HW) or tuple(a.shape) != (B, Cc):
        raise RuntimeError("ens_phase_accum: acc %s, m %s, a %s do not fit %d rows of %s" % (tuple(acc.shape), tuple(m.shape),
                                                                                             tuple(a.shape), k, tuple(y.shape)))
    if not (lab.is_cuda and lab.dtype == torch.int32 and acc.is_contiguous() and m.is_contiguous() and a.is_contiguous()):
        raise RuntimeError("ens_phase_accum: int32 device labels and contiguous tables")
    check_act(acc)
    _phase_span(lab, lstrides, k, B, 0, "ens_phase_accum: lab")
    _chk(lib().tmg_ens_phase_accum(c_vp(ptr), _i64(ps, co), _ptr(lab), _i64(*lstrides), _ptr(a), _ptr(m), _ptr(acc),
                                   _i64(k, B, HW, Cc, NB), _stream()), "tmg_ens_phase_accum")


def ens_budget_plan(S, B, Hh, Ww):
    """The launch plan of ens_budget_accum for S members of B cases of [3, H, W] (tmg_ens_budget_plan; nothing is launched) -> dict:
    tile pixels per block, tiles blocks per field (the grid is tiles x B), vec: True when the planes of the state are read and written
    with 16-byte accesses (W % 4 == 0 and an aligned state), ws = 0 workspace floats."""
    plan = (c_i64 * 4)()
    _chk(lib().tmg_ens_budget_plan(_i64(S, B, Hh, Ww), plan), "tmg_ens_budget_plan")
    tile, tiles, vec, ws = [int(v) for v in plan]
    return {"tile": tile, "tiles": tiles, "grid": (tiles, int(B)), "vec": bool(vec), "ws": ws}


def ens_budget_accum(y, a, m, raw, k, row0, t_before):
    """Add one chunk of k rows (y: NHWC [k*B, H, W, 3] or a channel-slice view, rows member-major) to the planes of the rows row0 ..
    row0 + k - 1 of the state raw [S + 1, B, 14, HW] (the target: k = 1, row0 = S), about the mean planes m [B, 3, HW] (None: 0) with
    the scales a [B, 3] (device fp32); t_before == 0 stores instead of adding (tmg_ens_budget_accum)."""
    kB, Hh, Ww, Cc = y.shape
    ptr, ps, co, _ = seg(y)
    check_device(y)
    check_act(raw)
    check_device(raw)
    check_act(a)
    R, B, Q, HW = raw.shape
    if Cc != 3 or Q != 14 or HW != Hh * Ww or kB != k * B or tuple(a.shape) != (B, 3) or (m is not None and tuple(m.shape) != (B, 3, HW)):
        raise RuntimeError("ens_budget_accum: raw %s, m %s, a %s do not fit %d rows of %s" % (
            tuple(raw.shape), None if m is None else tuple(m.shape), tuple(a.shape), k, tuple(y.shape)))
    if not (raw.is_contiguous() and a.is_contiguous() and (m is None or (m.is_contiguous() and m.is_cuda and m.dtype == torch.float32))):
        raise RuntimeError("ens_budget_accum: contiguous fp32 device tables")
    _chk(lib().tmg_ens_budget_accum(c_vp(ptr), _i64(ps, co), _ptr(a), _ptr(m), _ptr(raw), _i64(k, R - 1, B, Hh, Ww, row0, t_before),
                                    _stream()), "tmg_ens_budget_accum")


def ens_budget_terms(raw, M, fl, outs, member_budget, Hh, Ww, T):
    """The seven budget terms and the stresses of every row of the state raw [S + 1, B, 14, HW] after T timed steps: outs =
    (budget_mean, budget_std, target_budget [B, 7, HW], stress_mean, stress_std, target_stress [B, 3, HW]) fp32, member_budget
    [B, S, 7, HW] or None; M [B, 2, HW] fp64 the physical mean velocity, fl = (dx, dy, nu, rho) (tmg_ens_budget_terms)."""
    check_act(raw)
    check_device(raw)
    R, B, Q, HW = raw.shape
    if Q != 14 or HW != Hh * Ww or not raw.is_contiguous() or tuple(M.shape) != (B, 2, HW) or M.dtype != torch.float64 or \
            not (M.is_cuda and M.is_contiguous()) or len(fl) != 4 or len(outs) != 6:
        raise RuntimeError("ens_budget_terms: raw is [S + 1, B, 14, HW] fp32 and M [B, 2, HW] fp64 on the device, got %s and %s"
                           % (tuple(raw.shape), tuple(M.shape)))
    for t, n in zip(outs, (7, 7, 7, 3, 3, 3)):
        check_act(t)
        if tuple(t.shape) != (B, n, HW) or not t.is_contiguous():
            raise RuntimeError("ens_budget_terms: an output is %s, not a contiguous %s" % (tuple(t.shape), (B, n, HW)))
    if member_budget is not None:
        check_act(member_budget)
        if tuple(member_budget.shape) != (B, R - 1, 7, HW) or not member_budget.is_contiguous():
            raise RuntimeError("ens_budget_terms: member_budget is %s, not a contiguous %s" % (tuple(member_budget.shape), (B, R - 1, 7, HW)))
    _chk(lib().tmg_ens_budget_terms(_ptr(raw), _ptr(M), (ctypes.c_double * 4)(*[float(v) for v in fl]), *[_ptr(t) for t in outs],
                                    _ptr(member_budget), _i64(R - 1, B, Hh, Ww, T), _stream()), "tmg_ens_budget_terms")


def ens_flux_plan(S, B, Hh, Ww, widths):
    """The launch plan of ens_flux_accum for S members of B cases of [H, W] and the box widths `widths` (tmg_ens_flux_plan; nothing is
    launched) -> dict: tile (TH, TW) pixels per block, halo = r_max + 1, tiles (NTY, NTX) per field over the valid region of the
    smallest width, lds bytes of dynamic LDS, optin: True when that exceeds 64 KB, blocks = NTY NTX B per fed row.  A function of
    (H, W, widths); B only scales the blocks."""
    plan = (c_i64 * 8)()
    _chk(lib().tmg_ens_flux_plan(_i64(S, B, Hh, Ww, len(widths)), _i64(*widths), plan), "tmg_ens_flux_plan")
    th, tw, halo, nty, ntx, lds, optin, blocks = [int(v) for v in plan]
    return {"tile": (th, tw), "halo": halo, "tiles": (nty, ntx), "lds": lds, "optin": bool(optin), "blocks": blocks}


def ens_flux_accum(y, a, kk, raw, widths, k, row0, t_before):
    """Add one chunk of k rows (y: NHWC [k*B, H, W, 2..4] or a channel-slice view, rows member-major; channels 0 and 1 are read) to
    the planes of the rows row0 .. row0 + k - 1 of the state raw [S + 1, B, L, 7, HW] (the target: k = 1, row0 = S) with the scales
    a [B, 2] and the flux factors kk [L, 2] (device fp32); t_before == 0 stores instead of adding (tmg_ens_flux_accum)."""
    kB, Hh, Ww, Cc = y.shape
    ptr, ps, co, _ = seg(y)
    check_device(y)
    check_act(raw)
    check_device(raw)
    check_act(a)
    check_act(kk)
    if raw.dim() != 5:
        raise RuntimeError("ens_flux_accum: raw is [S + 1, B, L, 7, HW], got %s" % (tuple(raw.shape),))
    R, B, L, Q, HW = raw.shape
    if not 2 <= Cc <= 4 or Q != 7 or L != len(widths) or HW != Hh * Ww or kB != k * B or tuple(a.shape) != (B, 2) or tuple(kk.shape) != (L, 2):
        raise RuntimeError("ens_flux_accum: raw %s, a %s, kk %s do not fit %d rows of %s and %d widths" % (
            tuple(raw.shape), tuple(a.shape), tuple(kk.shape), k, tuple(y.shape), len(widths)))
    if not (raw.is_contiguous() and a.is_contiguous() and kk.is_contiguous()):
        raise RuntimeError("ens_flux_accum: contiguous fp32 device tables")
    _chk(lib().tmg_ens_flux_accum(c_vp(ptr), _i64(ps, co), _ptr(a), _ptr(kk), _ptr(raw), _i64(*widths),
                                  _i64(k, R - 1, B, Hh, Ww, row0, t_before, L), _stream()), "tmg_ens_flux_accum")


FLUX_OUTS = ("flux_mean", "flux_std", "target_flux", "flux_tstd_mean", "target_flux_tstd", "backscatter_mean", "backscatter_std",
             "target_backscatter", "sgs_mean", "sgs_std", "target_sgs", "member_flux", "flux_curve", "sgs_energy_curve")


def ens_flux_terms(raw, k64, outs, widths, Hh, Ww, T):
    """The time-mean flux, its temporal std, the backscatter fraction, the sub-filter stresses and the two curves of every row of the
    state raw [S + 1, B, L, 7, HW] after T timed steps: outs = the 14 arrays of FLUX_OUTS in that order (fp32 on the device; the
    fields [B, L, HW], the stresses [B, L, 3, HW], member_flux [B, S, L, HW] or None, the curves [B, S + 1, L]); k64 [L, 2] fp64 on the
    device (tmg_ens_flux_terms)."""
    check_act(raw)
    check_device(raw)
    if raw.dim() != 5 or raw.shape[3] != 7 or raw.shape[2] != len(widths) or raw.shape[4] != Hh * Ww or not raw.is_contiguous() or \
            len(outs) != len(FLUX_OUTS):
        raise RuntimeError("ens_flux_terms: raw is [S + 1, B, %d, 7, %d] fp32 on the device, got %s" % (len(widths), Hh * Ww, tuple(raw.shape)))
    R, B, L, _, HW = raw.shape
    if tuple(k64.shape) != (L, 2) or k64.dtype != torch.float64 or not (k64.is_cuda and k64.is_contiguous()):
        raise RuntimeError("ens_flux_terms: k64 is [L, 2] fp64 on the device, got %s" % (tuple(k64.shape),))
    want = [(B, L, HW)] * 8 + [(B, L, 3, HW)] * 3 + [(B, R - 1, L, HW)] + [(B, R, L)] * 2
    for name, t, shp in zip(FLUX_OUTS, outs, want):
        if t is None and name == "member_flux":
            continue
        check_act(t)
        if tuple(t.shape) != shp or not t.is_contiguous():
            raise RuntimeError("ens_flux_terms: %s is %s, not a contiguous %s" % (name, tuple(t.shape), shp))
    nw = 4 * ((HW + 255) // 256)
    ws = torch.empty((B * R * L * 2 * nw,), device=raw.device, dtype=torch.float64)
    table = (c_vp * len(outs))(*[None if t is None else t.data_ptr() for t in outs])
    _chk(lib().tmg_ens_flux_terms(_ptr(raw), _ptr(k64), table, _ptr(ws), _i64(*widths), _i64(R - 1, B, Hh, Ww, T, L), _stream()),
         "tmg_ens_flux_terms")


LAGR_OUTS = ("ftle_mean", "ftle_std", "target_ftle", "ftle_count", "disp_mean", "disp_std", "target_disp", "alive_frac", "target_alive",
             "res_time_mean", "res_time_std", "target_res_time", "end_err_mean", "end_spread", "member_ftle", "member_end", "member_exit")
LAGR_INT_OUTS = ("ftle_count", "member_exit")


def ens_lagr_seeds(lattice, boxes, substeps):
    """The host integers the advection and the finalize share: {Gh, Gw, oy, ox, sy, sx, R, n, then (h0, h1, w0, w1) of 4 boxes};
    lattice = (Gh, Gw, oy, ox, sy, sx)."""
    flat = [int(v) for v in lattice] + [len(boxes), int(substeps)]
    for r in range(4):
        flat += [int(v) for v in boxes[r]] if r < len(boxes) else [0, 0, 0, 0]
    return _i64(*flat)


def ens_lagr_steps(substeps):
    """The host floats of one advection of n = substeps Heun steps: s_j = float32(j / n), j = 0 .. 8 (0 past n), h = float32(1 / n),
    hh = float32(0.5 / n); each is one rounding of the fp64 quotient."""
    n = int(substeps)
    return _flts([j / n if j <= n else 0.0 for j in range(9)] + [1.0 / n, 0.5 / n])


def ens_lagr_plan(S, B, Hh, Ww, P):
    """The launch plans of ens_lagr_advect and ens_lagr_store for S members of B cases of [H, W] and P particles (tmg_ens_lagr_plan;
    nothing is launched) -> dict: tile particles per advect block, tiles blocks per row and case (the advect grid is tiles x B x k),
    store_tile pixels per store block, store_tiles blocks per row and case, vec: True when the planes of prev are written with
    16-byte stores (W % 4 == 0 and an aligned state), bytes of pos, exit and prev."""
    plan = (c_i64 * 6)()
    _chk(lib().tmg_ens_lagr_plan(_i64(S, B, Hh, Ww, P), plan), "tmg_ens_lagr_plan")
    tile, tiles, stile, stiles, vec, nbytes = [int(v) for v in plan]
    return {"tile": tile, "tiles": tiles, "grid": (tiles, int(B)), "store_tile": stile, "store_tiles": stiles, "vec": bool(vec),
            "bytes": nbytes}


def _lagr_feed(name, y, a, o, prev, k):
    kB, Hh, Ww, Cc = y.shape
    ptr, ps, co, _ = seg(y)
    check_device(y)
    check_act(prev)
    check_device(prev)
    check_act(a)
    check_act(o)
    if prev.dim() != 4:
        raise RuntimeError("%s: prev is [S + 1, B, 2, HW], got %s" % (name, tuple(prev.shape)))
    R, B, two, HW = prev.shape
    if not 2 <= Cc <= 4 or two != 2 or HW != Hh * Ww or kB != k * B or tuple(a.shape) != (B, 2) or tuple(o.shape) != (B, 2):
        raise RuntimeError("%s: prev %s, a %s, o %s do not fit %d rows of %s" % (name, tuple(prev.shape), tuple(a.shape), tuple(o.shape),
                                                                                k, tuple(y.shape)))
    if not (prev.is_contiguous() and a.is_contiguous() and o.is_contiguous()):
        raise RuntimeError("%s: contiguous fp32 device tables" % name)
    return ptr, ps, co, R, B, Hh, Ww


def ens_lagr_advect(y, a, o, prev, pos, exit_, res, lattice, boxes, substeps, k, row0, t_before):
    """Seed (t_before == 0) or advect by one kept step the particles of one chunk of k rows (y: NHWC [k*B, H, W, 2..4] or a
    channel-slice view, rows member-major; channels 0 and 1 are read): rows row0 .. row0 + k - 1 of the state pos [S + 1, B, 2, P]
    fp32, exit [S + 1, B, P] int32, res [S + 1, B, R, P] int32, through the planes prev [S + 1, B, 2, HW] of the previous timed step
    and the chunk's own rows, with the velocity tables a, o [B, 2] (device fp32) (tmg_ens_lagr_advect).  Before ens_lagr_store of the
    same rows, on the same stream."""
    ptr, ps, co, R, B, Hh, Ww = _lagr_feed("ens_lagr_advect", y, a, o, prev, k)
    P = int(lattice[0]) * int(lattice[1])
    check_act(pos)
    check_device(pos)
    for t, shp in ((exit_, (R, B, P)), (res, (R, B, len(boxes), P))):
        if not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()) or tuple(t.shape) != shp:
            raise RuntimeError("ens_lagr_advect: exit and res are contiguous int32 %s on the device, got %s %s" % (shp, t.dtype, tuple(t.shape)))
    if tuple(pos.shape) != (R, B, 2, P) or not pos.is_contiguous():
        raise RuntimeError("ens_lagr_advect: pos is %s, not a contiguous %s" % (tuple(pos.shape), (R, B, 2, P)))
    _chk(lib().tmg_ens_lagr_advect(c_vp(ptr), _i64(ps, co), _ptr(a), _ptr(o), _ptr(prev), _ptr(pos), _ptr(exit_), _ptr(res),
                                   ens_lagr_seeds(lattice, boxes, substeps), ens_lagr_steps(substeps),
                                   _i64(k, R - 1, B, Hh, Ww, row0, t_before), _stream()), "tmg_ens_lagr_advect")


def ens_lagr_store(y, a, o, prev, k, row0):
    """Write the converted velocity planes fl(fl(a y) + o) of one chunk of k rows into the rows row0 .. row0 + k - 1 of prev
    [S + 1, B, 2, HW] (tmg_ens_lagr_store).  After ens_lagr_advect of the same rows, on the same stream."""
    ptr, ps, co, R, B, Hh, Ww = _lagr_feed("ens_lagr_store", y, a, o, prev, k)
    _chk(lib().tmg_ens_lagr_store(c_vp(ptr), _i64(ps, co), _ptr(a), _ptr(o), _ptr(prev), _i64(k, R - 1, B, Hh, Ww, row0), _stream()),
         "tmg_ens_lagr_store")


def ens_lagr_finalize(pos, exit_, res, fl, outs, lattice, boxes, Hh, Ww):
    """The transport diagnostics of the state pos [S + 1, B, 2, P], exit [S + 1, B, P], res [S + 1, B, R, P]: outs = the 17 arrays of
    LAGR_OUTS in that order (fp32 on the device, ftle_count and member_exit int32; the res_time_* None without boxes, the member_*
    all three or None; shapes in include/tmglow_hip_lagr.h); fl = (dx, dy, step_dt, T_int) (tmg_ens_lagr_finalize)."""
    check_act(pos)
    check_device(pos)
    if pos.dim() != 4 or len(outs) != len(LAGR_OUTS) or len(fl) != 4:
        raise RuntimeError("ens_lagr_finalize: pos is [S + 1, B, 2, P] fp32 on the device, got %s" % (tuple(pos.shape),))
    R, B, two, P = pos.shape
    S, nb = R - 1, len(boxes)
    if two != 2 or P != int(lattice[0]) * int(lattice[1]) or not pos.is_contiguous():
        raise RuntimeError("ens_lagr_finalize: pos %s does not fit the lattice %s" % (tuple(pos.shape), tuple(lattice[:2])))
    for t, shp in ((exit_, (R, B, P)), (res, (R, B, nb, P))):
        if not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()) or tuple(t.shape) != shp:
            raise RuntimeError("ens_lagr_finalize: exit and res are contiguous int32 %s on the device, got %s %s" % (shp, t.dtype, tuple(t.shape)))
    want = [(B, P)] * 4 + [(B, 2, P)] * 3 + [(B, P)] * 2 + [(B, nb, P)] * 3 + [(B, P)] * 2 + [(B, S, P), (B, S, 2, P), (B, S, P)]
    for name, t, shp in zip(LAGR_OUTS, outs, want):
        if t is None and (name.startswith("member_") or (nb == 0 and "res_time" in name)):
            continue
        if t is None or not t.is_cuda or t.dtype != (torch.int32 if name in LAGR_INT_OUTS else torch.float32) or tuple(t.shape) != shp \
                or not t.is_contiguous():
            raise RuntimeError("ens_lagr_finalize: %s is not a contiguous %s device array of its type" % (name, shp))
    if len({outs[i] is None for i in (14, 15, 16)}) != 1:
        raise RuntimeError("ens_lagr_finalize: member_ftle, member_end and member_exit come all three or not at all")
    table = (c_vp * len(outs))(*[None if t is None else t.data_ptr() for t in outs])
    _chk(lib().tmg_ens_lagr_finalize(_ptr(pos), _ptr(exit_), _ptr(res), (ctypes.c_double * 4)(*[float(v) for v in fl]), table,
                                     ens_lagr_seeds(lattice, boxes, 1), _i64(S, B, Hh, Ww), _stream()), "tmg_ens_lagr_finalize")


VORTEX_PLAN_KEYS = ("TH", "TW", "NTH", "NTW", "tile_blocks", "merge_blocks", "pixel_blocks", "threads", "lds_label", "lds_census",
                    "ws_bytes", "state_bytes")
VORTEX_WORDS = 8


def ens_vortex_plan(k, S, B, Hh, Ww, K, Tn, code=False):
    """The launch plans of the vortex census for chunks of k rows of S members of B cases of [H, W], K table slots and Tn timed steps
    (tmg_ens_vortex_plan; nothing is launched) -> dict of VORTEX_PLAN_KEYS (include/tmglow_hip_vortex.h).  code=True: the C
    return code instead of raising (0 with the plan as second element)."""
    plan = (c_i64 * len(VORTEX_PLAN_KEYS))()
    rc = lib().tmg_ens_vortex_plan(_i64(k, S, B, Hh, Ww, K, Tn), plan)
    out = dict(zip(VORTEX_PLAN_KEYS, [int(v) for v in plan]))
    if code:
        return rc, out
    _chk(rc, "tmg_ens_vortex_plan")
    return out


def _vortex_planes(name, n, HW, dev, **planes):
    """Every plane is a contiguous [n, HW] device array of its dtype."""
    for key, (t, dt) in planes.items():
        if not t.is_cuda or t.dtype != dt or tuple(t.shape) != (n, HW) or not t.is_contiguous() or t.device != dev:
            raise RuntimeError("%s: %s is a contiguous [%d, %d] %s array on %s, got %s %s" % (name, key, n, HW, dt, dev, t.dtype, tuple(t.shape)))
        check_device(t)


def ens_vortex_classify(y, u, out_mu, out_std, thr, qscale, omega, cls, rejected, grid, k):
    """Classify one chunk of k rows (y: NHWC [k*B, H, W, 2..4] or a channel-slice view, rows member-major): omega [k*B, HW] fp32, cls
    [k*B, HW] int8 and rejected [k*B] int32 (set, not added to), with the device tables u [B, C] or None, out_mu, out_std [C], thr,
    qscale [B] and grid = (dx, dy) (tmg_ens_vortex_classify)."""
    kB, Hh, Ww, Cc = y.shape
    ptr, ps, co, _ = seg(y)
    check_device(y)
    B = kB // k
    _vortex_planes("ens_vortex_classify", kB, Hh * Ww, y.device, omega=(omega, torch.float32), cls=(cls, torch.int8))
    if kB != k * B or tuple(thr.shape) != (B,) or tuple(qscale.shape) != (B,) or rejected.dtype != torch.int32 or rejected.numel() != kB \
            or not rejected.is_contiguous() or (u is not None and tuple(u.shape) != (B, Cc)):
        raise RuntimeError("ens_vortex_classify: the tables do not fit %d rows of %s" % (k, tuple(y.shape)))
    for t in (u, out_mu, out_std, thr, qscale):
        if t is not None:
            check_act(t)
    _chk(lib().tmg_ens_vortex_classify(c_vp(ptr), _i64(ps, co), _ptr(u), _ptr(out_mu), _ptr(out_std), _ptr(thr), _ptr(qscale), _ptr(omega),
                                       _ptr(cls), _ptr(rejected), _flts(grid), _i64(k, B, Hh, Ww, Cc), _stream()), "tmg_ens_vortex_classify")


def ens_vortex_label(cls, label, status, Hh, Ww):
    """cls [n, HW] int8 -> label [n, HW] int32: the smallest linear index of the pixel's 4-connected component of one non-zero class,
    -1 on the background; status: one int32 on the device that receives a non-zero code when a loop reaches its trip bound
    (tmg_ens_vortex_label)."""
    n = cls.shape[0]
    _vortex_planes("ens_vortex_label", n, Hh * Ww, cls.device, cls=(cls, torch.int8), label=(label, torch.int32))
    if not status.is_cuda or status.dtype != torch.int32 or status.numel() != 1:
        raise RuntimeError("ens_vortex_label: status is one int32 on the device")
    _chk(lib().tmg_ens_vortex_label(_ptr(cls), _ptr(label), _ptr(status), _i64(n, Hh, Ww), _stream()), "tmg_ens_vortex_label")


def ens_vortex_census(label, cls, omega, qscale, area, slot, table, found, core, Hh, Ww, k, min_area):
    """The census of one chunk of k rows: label, cls, omega [k*B, HW] -> table [k*B, K, 8] int64 and found [k*B, 2] int32 (both
    overwritten) and core [B, 2, HW] int32 (added to); area, slot [k*B, HW] int32 are workspace (tmg_ens_vortex_census)."""
    kB, HW = label.shape
    B = kB // k
    i32 = torch.int32
    _vortex_planes("ens_vortex_census", kB, HW, label.device, label=(label, i32), cls=(cls, torch.int8), omega=(omega, torch.float32),
                   area=(area, i32), slot=(slot, i32))
    K = table.shape[1] if table.dim() == 3 else 0
    if HW != Hh * Ww or kB != k * B or table.dtype != torch.int64 or tuple(table.shape) != (kB, K, VORTEX_WORDS) or not table.is_contiguous() \
            or found.dtype != i32 or tuple(found.shape) != (kB, 2) or not found.is_contiguous() or core.dtype != i32 \
            or tuple(core.shape) != (B, 2, HW) or not core.is_contiguous() or tuple(qscale.shape) != (B,):
        raise RuntimeError("ens_vortex_census: table %s, found %s, core %s do not fit %d rows of %d cases of %d pixels"
                           % (tuple(table.shape), tuple(found.shape), tuple(core.shape), k, B, HW))
    check_act(qscale)
    _chk(lib().tmg_ens_vortex_census(_ptr(label), _ptr(cls), _ptr(omega), _ptr(qscale), _ptr(area), _ptr(slot), _ptr(table), _ptr(found),
                                     _ptr(core), _i64(k, B, Hh, Ww, K, min_area), _stream()), "tmg_ens_vortex_census")


FRANK_PLAN_KEYS = ("nblk", "grid_x", "grid_y", "grid_z", "threads", "rec_words", "ws_words")


def ens_frank_plan(S, B, C, HW, code=False):
    """The launch plan of ens_frank_step for S members and the target of B cases of [C, HW] (tmg_ens_frank_plan; nothing is
    launched) -> dict of FRANK_PLAN_KEYS (include/tmglow_hip_frank.h) plus grid = (nblk, C, B).  code=True: the C return code
    instead of raising, as the second element of a pair."""
    plan = (c_i64 * len(FRANK_PLAN_KEYS))()
    rc = lib().tmg_ens_frank_plan(_i64(S, B, C, HW), plan)
    out = dict(zip(FRANK_PLAN_KEYS, [int(v) for v in plan]))
    out["grid"] = (out["grid_x"], out["grid_y"], out["grid_z"])
    if code:
        return out, rc
    _chk(rc, "tmg_ens_frank_plan")
    return out


def ens_frank_step(xs, ws, pre_raw, outside, tout, t, t_before, flags):
    """The average-rank and band-depth terms of one kept step whose S members and target are the rows of xs [S + 1, B, C, HW] (the
    target last): their sums over the pixels into pre_raw [B, Tk, C, S + 1, 2] int64 and the count of pixels whose target lies
    strictly outside the members' range into outside [B, Tk, C] int64, both at step t; ws: the int32 workspace (>= ens_frank_plan's
    words).  flags & 1 adds the outside flags to the plane tout [B, C, HW] int32, which holds t_before steps (tmg_ens_frank_step)."""
    R, B, Cc, HW = xs.shape
    i32, i64 = torch.int32, torch.int64
    if xs.dtype != torch.float32 or not xs.is_cuda or not xs.is_contiguous() or R < 2:
        raise RuntimeError("ens_frank_step: xs is a contiguous fp32 [S + 1, B, C, HW] on the device, got %s %s" % (xs.dtype, tuple(xs.shape)))
    check_device(xs)
    Tk = pre_raw.shape[1] if pre_raw.dim() == 5 else 0
    if pre_raw.dtype != i64 or tuple(pre_raw.shape) != (B, Tk, Cc, R, 2) or not pre_raw.is_contiguous() or outside.dtype != i64 \
            or tuple(outside.shape) != (B, Tk, Cc) or not outside.is_contiguous() or ws.dtype != i32 or ws.dim() != 1 \
            or not ws.is_contiguous() or pre_raw.device != xs.device or outside.device != xs.device or ws.device != xs.device:
        raise RuntimeError("ens_frank_step: pre_raw %s, outside %s, ws %s do not fit %d rows of [%d, %d, %d]"
                           % (tuple(pre_raw.shape), tuple(outside.shape), tuple(ws.shape), R, B, Cc, HW))
    if tout is not None and (tout.dtype != i32 or tuple(tout.shape) != (B, Cc, HW) or not tout.is_contiguous() or tout.device != xs.device):
        raise RuntimeError("ens_frank_step: tout is a contiguous int32 [%d, %d, %d] on the device, got %s" % (B, Cc, HW, tuple(tout.shape)))
    _chk(lib().tmg_ens_frank_step(_ptr(xs), _ptr(ws), ws.numel(), _ptr(pre_raw), _ptr(outside), _ptr(tout),
                                  _i64(R - 1, B, HW, Cc, Tk, t, t_before, flags), _stream()), "tmg_ens_frank_step")


SPELL_PLAN_KEYS = ("blocks", "threads", "group", "lds_bytes", "state_words", "grid_x", "grid_y", "row_words", "table_words", "fin_lds_bytes")
SPELL_MAPS = 7


def ens_spell_plan(S, B, HW, K, L, Tn, code=False):
    """The launch plan of ens_spell_step / ens_spell_finalize for S members and the target of B cases of HW pixels, K events, L length
    bins and a window of Tn steps (tmg_ens_spell_plan; nothing is launched) -> dict of SPELL_PLAN_KEYS (include/tmglow_hip_spell.h)
    plus grid = (grid_x, grid_y).  code=True: the C return code instead of raising, as the second element of a pair."""
    plan = (c_i64 * len(SPELL_PLAN_KEYS))()
    rc = lib().tmg_ens_spell_plan(_i64(S, B, HW, K, L, Tn), plan)
    out = dict(zip(SPELL_PLAN_KEYS, [int(v) for v in plan]))
    out["grid"] = (out["grid_x"], out["grid_y"])
    if code:
        return out, rc
    _chk(rc, "tmg_ens_spell_plan")
    return out


def _spell_buffers(name, state, table, maps, S, B, K, HW, dev):
    """state [S + 1, B, K, HW] int32, table [B, K, S + 1, 2, L + 7] int64, maps [7, B, K, HW] int32, contiguous on dev -> L."""
    L = table.shape[4] - 7 if table.dim() == 5 else 0
    for key, t, dt, shape in (("state", state, torch.int32, (S + 1, B, K, HW)), ("table", table, torch.int64, (B, K, S + 1, 2, L + 7)),
                              ("maps", maps, torch.int32, (SPELL_MAPS, B, K, HW))):
        if not t.is_cuda or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev:
            raise RuntimeError("%s: %s is a contiguous %s %s array on %s, got %s %s" % (name, key, list(shape), dt, dev, t.dtype, tuple(t.shape)))
        check_device(t)
    return L


def ens_spell_step(y, thr, ev, state, table, maps, S, k, row0, Tn, t, code=False):
    """Advance the run-length state of one chunk of k rows (y: NHWC [k*B, H, W, C] or a channel-slice view, rows member-major) by
    window step t of Tn against the K events ev = ((channel, 1 for > / 0 for <), ..) with the raw thresholds thr [B, K] (device):
    rows row0 .. row0 + k - 1 of the S members, or the target as the one-row chunk row0 = S.  state [S + 1, B, K, HW] int32 (step 0
    writes it), table [B, K, S + 1, 2, L + 7] int64 (the call of step 0 with row0 = 0 zeroes it) and maps [7, B, K, HW] int32 as in
    include/tmglow_hip_spell.h (tmg_ens_spell_step).  code=True: the C return code instead of raising."""
    kB, Hh, Ww, Cc = y.shape
    ptr, ps, co, _ = seg(y)
    check_device(y)
    B, K = kB // max(k, 1), len(ev)
    L = _spell_buffers("ens_spell_step", state, table, maps, S, B, K, Hh * Ww, y.device)
    if thr.dtype != torch.float32 or tuple(thr.shape) != (B, K) or not thr.is_contiguous() or thr.device != y.device:
        raise RuntimeError("ens_spell_step: thr is a contiguous fp32 [%d, %d] on %s, got %s %s" % (B, K, y.device, thr.dtype, tuple(thr.shape)))
    evf = [int(v) for e in ev for v in e]
    rc = lib().tmg_ens_spell_step(c_vp(ptr), _i64(ps, co), _ptr(thr), _i64(*evf) if evf else None, _ptr(state), _ptr(table), _ptr(maps),
                                  _i64(k, B, Hh * Ww, Cc, S, row0, K, L, Tn, t), _stream())
    if code:
        return rc
    _chk(rc, "tmg_ens_spell_step")


def ens_spell_finalize(state, table, maps, Tn, code=False):
    """Once, after the last step of every row: count the runs that are still open as right or both into table and fold every row's
    longest spell into maps planes 2, 3 and 6 (tmg_ens_spell_finalize).  code=True: the C return code instead of raising."""
    R, B, K, HW = state.shape
    L = _spell_buffers("ens_spell_finalize", state, table, maps, R - 1, B, K, HW, state.device)
    rc = lib().tmg_ens_spell_finalize(_ptr(state), _ptr(table), _ptr(maps), _i64(R - 1, B, HW, K, L, Tn), _stream())
    if code:
        return rc
    _chk(rc, "tmg_ens_spell_finalize")


ISCALE_PLAN_KEYS = ("tile", "tiles_x", "tiles_y", "grid_x", "grid_y", "grid_z", "blocks", "threads", "group", "lds_bytes", "step_lds_bytes",
                    "member_words", "target_words", "ens_words")


def ens_iscale_plan(S, B, H, W, K, L, code=False):
    """The launch plan of ens_iscale_chunk / ens_iscale_step for S members of B cases of [H, W], K events and L Haar levels
    (tmg_ens_iscale_plan; nothing is launched) -> dict of ISCALE_PLAN_KEYS (include/tmglow_hip_iscale.h) plus grid = (grid_x, grid_y,
    grid_z).  code=True: the C return code instead of raising, as the second element of a pair."""
    plan = (c_i64 * len(ISCALE_PLAN_KEYS))()
    rc = lib().tmg_ens_iscale_plan(_i64(S, B, H, W, K, L), plan)
    out = dict(zip(ISCALE_PLAN_KEYS, [int(v) for v in plan]))
    out["grid"] = (out["grid_x"], out["grid_y"], out["grid_z"])
    if code:
        return out, rc
    _chk(rc, "tmg_ens_iscale_plan")
    return out


def _iscale_buffers(name, bufs, dev):
    """bufs: (key, tensor, dtype, shape) entries, each a contiguous array of that dtype and shape on dev."""
    for key, t, dt, shape in bufs:
        if not t.is_cuda or t.dtype != dt or tuple(t.shape) != tuple(shape) or not t.is_contiguous() or t.device != dev:
            raise RuntimeError("%s: %s is a contiguous %s %s array on %s, got %s %s" % (name, key, list(shape), dt, dev, t.dtype, tuple(t.shape)))
        check_device(t)


def _iscale_thr(name, thr, B, K, dev):
    if thr.dtype != torch.float32 or tuple(thr.shape) != (B, K) or not thr.is_contiguous() or thr.device != dev:
        raise RuntimeError("%s: thr is a contiguous fp32 [%d, %d] on %s, got %s %s" % (name, B, K, dev, thr.dtype, tuple(thr.shape)))


def ens_iscale_chunk(y, target, thr, ev, cnt, member, target_tab, ens, S, k, m0, code=False):
    """The block-count sums of one chunk of k members (y: NHWC [k*B, H, W, C] or a channel-slice view, rows member-major) against the
    step's target (NHWC [B, H, W, C] or a channel-slice view) for the K events ev = ((channel, 1 for > / 0 for <), ..) with the raw
    thresholds thr [B, K] (device): (A, X) of the members m0 .. m0 + k - 1 into member [B, K, S, L + 1, 2] int64, their indicators
    into cnt [B, K, HW] int32 (m0 = 0 writes, later chunks add); the call with m0 = 0 zeroes member, target_tab [B, K, L + 1] and ens
    [B, K, L + 1, 2] first and adds Cc into target_tab (tmg_ens_iscale_chunk, include/tmglow_hip_iscale.h).  code=True: the C return
    code instead of raising."""
    kB, Hh, Ww, Cc = y.shape
    ptr, ps, co, _ = seg(y)
    tptr, tps, tco, _ = seg(target)
    check_device(y)
    check_device(target)
    B, K = kB // max(k, 1), len(ev)
    L = ens.shape[2] - 1 if ens.dim() == 4 else 0
    _iscale_buffers("ens_iscale_chunk", (("cnt", cnt, torch.int32, (B, K, Hh * Ww)), ("member", member, torch.int64, (B, K, S, L + 1, 2)),
                                         ("target_tab", target_tab, torch.int64, (B, K, L + 1)), ("ens", ens, torch.int64, (B, K, L + 1, 2))),
                    y.device)
    _iscale_thr("ens_iscale_chunk", thr, B, K, y.device)
    if tuple(target.shape) != (B, Hh, Ww, Cc) or target.device != y.device:
        raise RuntimeError("ens_iscale_chunk: target is [%d, %d, %d, %d] on %s, got %s" % (B, Hh, Ww, Cc, y.device, tuple(target.shape)))
    evf = [int(v) for e in ev for v in e]
    rc = lib().tmg_ens_iscale_chunk(c_vp(ptr), _i64(ps, co), c_vp(tptr), _i64(tps, tco), _ptr(thr), _i64(*evf) if evf else None, _ptr(cnt),
                                    _ptr(member), _ptr(target_tab), _ptr(ens), _i64(k, B, Hh, Ww, Cc, S, m0, K, L), _stream())
    if code:
        return rc
    _chk(rc, "tmg_ens_iscale_chunk")


def ens_iscale_step(cnt, target, thr, ev, ens, S, code=False):
    """Once per kept step, after its last chunk: (AN, XN) of the member counts cnt [B, K, HW] int32 against target (NHWC [B, H, W, C]
    or a channel-slice view) into ens [B, K, L + 1, 2] int64 (tmg_ens_iscale_step).  code=True: the C return code instead of raising."""
    B, Hh, Ww, Cc = target.shape
    tptr, tps, tco, _ = seg(target)
    check_device(target)
    K = len(ev)
    L = ens.shape[2] - 1 if ens.dim() == 4 else 0
    _iscale_buffers("ens_iscale_step", (("cnt", cnt, torch.int32, (B, K, Hh * Ww)), ("ens", ens, torch.int64, (B, K, L + 1, 2))), target.device)
    _iscale_thr("ens_iscale_step", thr, B, K, target.device)
    evf = [int(v) for e in ev for v in e]
    rc = lib().tmg_ens_iscale_step(_ptr(cnt), c_vp(tptr), _i64(tps, tco), _ptr(thr), _i64(*evf) if evf else None, _ptr(ens),
                                   _i64(S, B, Hh, Ww, Cc, K, L), _stream())
    if code:
        return rc
    _chk(rc, "tmg_ens_iscale_step")


MINK_PLAN_KEYS = ("tile_h", "tile_w", "tiles_x", "tiles_y", "grid_x", "grid_y", "grid_z", "blocks", "threads", "group", "lds_bytes",
                  "table_words")


def ens_mink_plan(S, B, H, W, F, J, code=False):
    """The launch plan of ens_mink_chunk for S members of B cases of [H, W], F fields and a ladder of J levels (tmg_ens_mink_plan;
    nothing is launched) -> dict of MINK_PLAN_KEYS (include/tmglow_hip_mink.h) plus grid = (grid_x, grid_y, grid_z).  code=True: the
    C return code instead of raising, as the second element of a pair."""
    plan = (c_i64 * len(MINK_PLAN_KEYS))()
    rc = lib().tmg_ens_mink_plan(_i64(S, B, H, W, F, J), plan)
    out = dict(zip(MINK_PLAN_KEYS, [int(v) for v in plan]))
    out["grid"] = (out["grid_x"], out["grid_y"], out["grid_z"])
    if code:
        return out, rc
    _chk(rc, "tmg_ens_mink_plan")
    return out


def ens_mink_chunk(y, target, thr, fields, table, S, k, m0, code=False):
    """The excursion-set counts of one chunk of k members (y: NHWC [k*B, H, W, C] or a channel-slice view, rows member-major) and,
    with m0 = 0, of the step's target (NHWC [B, H, W, C] or a channel-slice view) for the channels `fields` against the raw ladders
    thr [B, F, J] (device): (N, Nh, Nv, Nq, Nd) of the members m0 .. m0 + k - 1 into their rows of table [B, F, S + 1, J, 5] int64;
    the call with m0 = 0 zeroes the whole table first and adds the target's row S (tmg_ens_mink_chunk, include/tmglow_hip_mink.h).
    code=True: the C return code instead of raising."""
    kB, Hh, Ww, Cc = y.shape
    ptr, ps, co, _ = seg(y)
    tptr, tps, tco, _ = seg(target)
    check_device(y)
    check_device(target)
    B, F = kB // max(k, 1), len(fields)
    J = thr.shape[2] if thr.dim() == 3 else 0
    _iscale_buffers("ens_mink_chunk", (("table", table, torch.int64, (B, F, S + 1, J, 5)), ("thr", thr, torch.float32, (B, F, J))), y.device)
    if tuple(target.shape) != (B, Hh, Ww, Cc) or target.device != y.device:
        raise RuntimeError("ens_mink_chunk: target is [%d, %d, %d, %d] on %s, got %s" % (B, Hh, Ww, Cc, y.device, tuple(target.shape)))
    ff = [int(v) for v in fields]
    rc = lib().tmg_ens_mink_chunk(c_vp(ptr), _i64(ps, co), c_vp(tptr), _i64(tps, tco), _ptr(thr), _i64(*ff) if ff else None, _ptr(table),
                                  _i64(k, B, Hh, Ww, Cc, S, m0, F, J), _stream())
    if code:
        return rc
    _chk(rc, "tmg_ens_mink_chunk")


EDT_PLAN_KEYS = ("tile_w", "band", "strips", "bands", "grid_x", "grid_y", "grid_z", "blocks", "threads", "lds_bytes", "mask_grid_x",
                 "scratch_words", "pair_words", "hist_words", "count_words", "map_words")


def ens_edt_plan(S, B, H, W, K, c, code=False):
    """The launch plan of ens_edt_chunk for S members of B cases of [H, W], K events and the cutoff c (tmg_ens_edt_plan; nothing is
    launched) -> dict of EDT_PLAN_KEYS (include/tmglow_hip_edt.h) plus grid = (grid_x, grid_y, grid_z).  code=True: the C return
    code instead of raising, as the second element of a pair."""
    plan = (c_i64 * len(EDT_PLAN_KEYS))()
    rc = lib().tmg_ens_edt_plan(_i64(S, B, H, W, K, c), plan)
    out = dict(zip(EDT_PLAN_KEYS, [int(v) for v in plan]))
    out["grid"] = (out["grid_x"], out["grid_y"], out["grid_z"])
    if code:
        return out, rc
    _chk(rc, "tmg_ens_edt_plan")
    return out


def ens_edt_chunk(y, target, thr, ev, scratch, count, dmap, msum, pair, hist, S, k, m0, code=False):
    """The distance-map sums of one chunk of k members (y: NHWC [k*B, H, W, C] or a channel-slice view, rows member-major) against
    the step's target (NHWC [B, H, W, C] or a channel-slice view) for the K events ev = ((channel, 1 for > / 0 for <), ..) with the
    raw thresholds thr [B, K] (device): the eleven sums of the members m0 .. m0 + k - 1 into pair [B, K, S, 11] int64, their
    histograms into hist [B, K, S, 2, c + 1] int64, their fixed-point distances into msum [B, K, HW] int32; scratch holds the
    indicator words [S + 1, B, K, H, ceil(W / 64)] int64 and count [B, K, S + 1] int32 the set sizes.  The call with m0 = 0 presets
    pair, hist, count and msum first and writes the target's squared distances into dmap [B, K, HW] int32 (tmg_ens_edt_chunk,
    include/tmglow_hip_edt.h).  code=True: the C return code instead of raising."""
    kB, Hh, Ww, Cc = y.shape
    ptr, ps, co, _ = seg(y)
    tptr, tps, tco, _ = seg(target)
    check_device(y)
    check_device(target)
    B, K = kB // max(k, 1), len(ev)
    c = hist.shape[4] - 1 if hist.dim() == 5 else 0
    _iscale_buffers("ens_edt_chunk", (("scratch", scratch, torch.int64, (S + 1, B, K, Hh, (Ww + 63) // 64)),
                                      ("count", count, torch.int32, (B, K, S + 1)), ("dmap", dmap, torch.int32, (B, K, Hh * Ww)),
                                      ("msum", msum, torch.int32, (B, K, Hh * Ww)), ("pair", pair, torch.int64, (B, K, S, 11)),
                                      ("hist", hist, torch.int64, (B, K, S, 2, c + 1))), y.device)
    _iscale_thr("ens_edt_chunk", thr, B, K, y.device)
    if tuple(target.shape) != (B, Hh, Ww, Cc) or target.device != y.device:
        raise RuntimeError("ens_edt_chunk: target is [%d, %d, %d, %d] on %s, got %s" % (B, Hh, Ww, Cc, y.device, tuple(target.shape)))
    evf = [int(v) for e in ev for v in e]
    rc = lib().tmg_ens_edt_chunk(c_vp(ptr), _i64(ps, co), c_vp(tptr), _i64(tps, tco), _ptr(thr), _i64(*evf) if evf else None, _ptr(scratch),
                                 _ptr(count), _ptr(dmap), _ptr(msum), _ptr(pair), _ptr(hist), _i64(k, B, Hh, Ww, Cc, S, m0, K, c), _stream())
    if code:
        return rc
    _chk(rc, "tmg_ens_edt_chunk")


def ens_edt_step(msum, dmap, tmem, ttgt, H, W, c, code=False):
    """Once per step that counts for the time maps, after its last chunk: tmem += msum and ttgt += w(dmap), all [B, K, H W], the
    sums int64 (tmg_ens_edt_step).  code=True: the C return code instead of raising."""
    B, K = (msum.shape[0], msum.shape[1]) if msum.dim() == 3 else (0, 0)
    shape = (B, K, H * W)
    _iscale_buffers("ens_edt_step", (("msum", msum, torch.int32, shape), ("dmap", dmap, torch.int32, shape),
                                     ("tmem", tmem, torch.int64, shape), ("ttgt", ttgt, torch.int64, shape)), msum.device)
    rc = lib().tmg_ens_edt_step(_ptr(msum), _ptr(dmap), _ptr(tmem), _ptr(ttgt), _i64(B, H, W, K, c), _stream())
    if code:
        return rc
    _chk(rc, "tmg_ens_edt_step")


def ens_edt_fixed(d2, c):
    """The kernels' fixed-point distance on the host (tmg_ens_edt_fixed; no device): d2, a sequence of integers in 0 .. 2^30, and the
    cutoff c -> the list of w = 256 c if d2 >= c^2 else isqrt(65536 d2), through the kernels' own float estimate and integer fix-up."""
    v = [int(x) for x in d2]
    out = (c_i64 * max(len(v), 1))()
    _chk(lib().tmg_ens_edt_fixed(_i64(*v) if v else (c_i64 * 1)(), len(v), int(c), out), "tmg_ens_edt_fixed")
    return [int(out[i]) for i in range(len(v))]


LSPEC_PLAN_KEYS = ("tiles", "mode_tiles", "grid_x", "grid_y", "threads", "lds_bytes", "nq", "nqp", "part_floats", "mean_floats",
                   "comom_floats", "operand_floats")


def ens_lspec_plan(k, S, B, C, L, N, code=False):
    """The launch plan and buffer sizes of ens_lspec_chunk for a chunk of k of S members of B cases, C channels, L lines of N points
    (tmg_ens_lspec_plan; nothing is launched) -> dict of LSPEC_PLAN_KEYS (include/tmglow_hip_lspec.h).  code=True: the C return code
    instead of raising, as the second element of a pair."""
    plan = (c_i64 * len(LSPEC_PLAN_KEYS))()
    rc = lib().tmg_ens_lspec_plan(_i64(k, S, B, C, L, N), plan)
    out = dict(zip(LSPEC_PLAN_KEYS, [int(v) for v in plan]))
    if code:
        return out, rc
    _chk(rc, "tmg_ens_lspec_plan")
    return out


def _lspec_f32(name, bufs, dev):
    for what, t in bufs:
        if t is not None and (t.dtype != torch.float32 or t.device != dev or not t.is_contiguous()):
            raise RuntimeError("%s: %s must be a contiguous fp32 tensor on %s" % (name, what, dev))


def ens_lspec_chunk(y, u, out_mu, out_std, op, mean, comom, part, S, k, m0, t_before, timed, columns=False, code=False):
    """The line transforms of one chunk of k members (y: NHWC [k*B, H, W, C] or a channel-slice view, rows member-major): lines are
    the rows of an image (L = H, N = W), or its columns with columns=True (L = W, N = H).  op [2, N, NQP]: the operand; part
    [>= k*B*tiles*F*NQ]: the tiles' line sums of the planes of X; timed: the running means mean [S, B, C, L, NQ, 2] and the co-moments
    comom [S, B, F, L, NQ] of the members m0 .. m0 + k - 1 take one more step (t_before: the steps they hold)
    (tmg_ens_lspec_chunk, include/tmglow_hip_lspec.h).  code=True: the C return code instead of raising."""
    kB, Hh, Ww, Cc = y.shape
    ptr, ps, co, _ = seg(y)
    check_device(y)
    _lspec_f32("ens_lspec_chunk", (("u", u), ("out_mu", out_mu), ("out_std", out_std), ("op", op), ("mean", mean), ("comom", comom),
                                   ("part", part)), y.device)
    B = kB // max(k, 1)
    L, N, ls, pstr = (Ww, Hh, 1, Ww) if columns else (Hh, Ww, Ww, 1)
    rc = lib().tmg_ens_lspec_chunk(c_vp(ptr), _i64(ps, co), _ptr(u), _ptr(out_mu), _ptr(out_std), _ptr(op), _ptr(mean), _ptr(comom),
                                   _ptr(part), _i64(k, S, B, Cc, L, N, ls, pstr, m0, t_before, 1 if timed else 0, part.numel(),
                                                    0 if mean is None else mean.numel(), 0 if comom is None else comom.numel(),
                                                    op.numel()), _stream())
    if code:
        return rc
    _chk(rc, "tmg_ens_lspec_chunk")


def ens_lspec_step(part, state, mean_out, std_out, k, L, N, n_before, S, t, last, code=False):
    """Fold one chunk's partials (ens_lspec_chunk) into the step's statistics over the members: state [2, B, F, NQ] is the
    sequential Welford's (mean, M2); last: the mean and the population std go to mean_out / std_out [B, Tk, F, NQ] at step t
    (tmg_ens_lspec_step).  code=True: the C return code instead of raising."""
    _, B, F, _ = state.shape
    Tk = mean_out.shape[1]
    _lspec_f32("ens_lspec_step", (("part", part), ("state", state), ("mean_out", mean_out), ("std_out", std_out)), part.device)
    rc = lib().tmg_ens_lspec_step(_ptr(part), _ptr(state), _ptr(mean_out), _ptr(std_out),
                                  _i64(k, B, F, L, N, n_before, S, Tk, t, 1 if last else 0), _stream())
    if code:
        return rc
    _chk(rc, "tmg_ens_lspec_step")


def ens_lspec_finalize(mean, comom, outs, member_out, T, code=False):
    """Mean and population std over the members of the fluctuation and of the mean-flow spectra from the members' state (mean
    [S, B, C, L, NQ, 2], comom [S, B, F, L, NQ]) after T timed steps -> outs = (fluct_mean, fluct_std, flow_mean, flow_std), each
    [B, F, L, NQ]; member_out [B, S, F, L, NQ] or None (tmg_ens_lspec_finalize).  code=True: the C return code instead of raising."""
    S, B, C, L, NQ, _ = mean.shape
    _lspec_f32("ens_lspec_finalize", (("mean", mean), ("comom", comom), ("member_out", member_out)) + tuple(("out", o) for o in outs),
               mean.device)
    rc = lib().tmg_ens_lspec_finalize(_ptr(mean), _ptr(comom), *[_ptr(o) for o in outs], _ptr(member_out),
                                      _i64(S, B, C, L, 2 * (NQ - 1), T), _stream())
    if code:
        return rc
    _chk(rc, "tmg_ens_lspec_finalize")


XSPEC_PLAN_KEYS = ("prep_grid", "cols_grid_x", "cols_grid_y", "cols_lds_bytes", "accum_grid_x", "accum_grid_y", "threads", "f_floats",
                   "part_floats", "zt_floats", "part_t_floats")


def ens_xspec_plan(k, B, Hh, Ww, NK, code=False):
    """The grids, LDS bytes and buffer sizes of the spectral-skill launches for a chunk of k members of B cases of [H, W] with NK
    shells (tmg_ens_xspec_plan; nothing is launched) -> dict of XSPEC_PLAN_KEYS (include/tmglow_hip_xspec.h).  code=True: the C
    return code instead of raising, as the second element of a pair."""
    plan = (c_i64 * len(XSPEC_PLAN_KEYS))()
    rc = lib().tmg_ens_xspec_plan(_i64(k, B, Hh, Ww, NK), plan)
    out = dict(zip(XSPEC_PLAN_KEYS, [int(v) for v in plan]))
    if code:
        return out, rc
    _chk(rc, "tmg_ens_xspec_plan")
    return out


def ens_xspec_prep(y, u, out_mu, out_std, center, f, fsum, k, mode, S):
    """f = u fmaf(out_std, y, out_mu) - center of channels 0 and 1 of the chunk's k members (y: NHWC [k*B, H, W, C] or a channel-slice
    view) into the dense f [>= k*B, H, W, 2]; mode 0: f alone (the target), 1 / 2: the members also go into fsum [B, H, W, 2] (1: the
    step's first chunk stores), 3: f = fsum / S, y is None (tmg_ens_xspec_prep)."""
    B, Hh, Ww, _ = fsum.shape
    if mode == 3:
        ptr, ps, co, Cc = 0, 0, 0, 2
    else:
        ptr, ps, co, Cc = seg(y)
    _chk(lib().tmg_ens_xspec_prep(c_vp(ptr), _i64(ps, co), _ptr(u), _ptr(out_mu), _ptr(out_std), _ptr(center), _ptr(f), _ptr(fsum),
                                  _i64(k, B, Hh, Ww, Cc, mode, S, f.numel()), _stream()), "tmg_ens_xspec_prep")


def ens_xspec_cols(ft_h, yw, perm, offs, zt, part, n, B, Hh, Ww, NK, cross):
    """Column transform of the n images in yw (ft_h: [2, H, H]) and the shell sums of every 16-column tile in the order of the tiles'
    shell lists (perm, offs).  cross False (n = B, the target): Z into zt [2, B, H, W], the sums of P into part [B, W/16, NK];
    cross True: (P, X, D) against zt into part [n, W/16, 3, NK] (tmg_ens_xspec_cols)."""
    _chk(lib().tmg_ens_xspec_cols(_ptr(ft_h), _ptr(yw), _ptr(perm), _ptr(offs), _ptr(zt), _ptr(part),
                                  _i64(n, B, Hh, Ww, NK, 1 if cross else 0, yw.numel(), zt.numel(), part.numel()),
                                  _flts([0.5 / (float(Hh) * float(Ww)) ** 2]), _stream()), "tmg_ens_xspec_cols")


def ens_xspec_accum(part, part_t, part_b, step, tpow, sum_out, bar_out, tmem, ttgt, tbar, k, QT, t, n_before, m0, t_before, flags):
    """Fold one chunk's partial sums (ens_xspec_cols) into the step sums `step` [B, 3, NK], the members' time sums tmem [B, S, 3, NK],
    and at the step's first / last chunk the target's and the mean field's sums into tpow [B, Tk, NK], ttgt [B, NK], bar_out and
    sum_out [B, Tk, 3, NK], tbar [B, 3, NK]; flags: 1 timed, 2 last (tmg_ens_xspec_accum)."""
    B, S, _, NK = tmem.shape
    Tk = tpow.shape[1]
    _chk(lib().tmg_ens_xspec_accum(_ptr(part), _ptr(part_t), _ptr(part_b), _ptr(step), _ptr(tpow), _ptr(sum_out), _ptr(bar_out),
                                   _ptr(tmem), _ptr(ttgt), _ptr(tbar), _i64(k, B, NK, QT, S, Tk, t, n_before, m0, t_before, flags),
                                   _stream()), "tmg_ens_xspec_accum")


def ens_corr_cfg(probes, pairs, lags):
    """The host integers the three correlation launches share: {P, Q, L, (h, w) of every probe, (ci, cj) of every pair, the lags}."""
    flat = [len(probes), len(pairs), len(lags)]
    for hw in probes:
        flat += [hw[0], hw[1]]
    for cc in pairs:
        flat += [cc[0], cc[1]]
    return _i64(*(flat + list(lags)))


def ens_corr_plan(S, B, Hh, Ww, P, Q, L, J):
    """The launch plan of ens_corr_accum for S members of B cases of [3, H, W], P probes, Q channel pairs, L lags and J distinct field
    channels (tmg_ens_corr_plan; nothing is launched) -> dict: tile pixels per block, tiles blocks per field (the grid is tiles x B),
    vec: True when the planes of the state are read and written with 16-byte accesses (W % 4 == 0 and an aligned state), planes =
    P Q L + 2 J L the planes of one row and case, offX, offF, offG the first plane of each kind, ws = 0 workspace floats."""
    plan = (c_i64 * 8)()
    _chk(lib().tmg_ens_corr_plan(_i64(S, B, Hh, Ww, P, Q, L, J), plan), "tmg_ens_corr_plan")
    tile, tiles, vec, npl, offx, offf, offg, ws = [int(v) for v in plan]
    return {"tile": tile, "tiles": tiles, "grid": (tiles, int(B)), "vec": bool(vec), "planes": npl, "offX": offx, "offF": offf,
            "offG": offg, "ws": ws}


def _corr_feed(name, y, a, m, series, k, P):
    kB, Hh, Ww, Cc = y.shape
    ptr, ps, co, _ = seg(y)
    check_device(y)
    check_act(series)
    check_device(series)
    check_act(a)
    if series.dim() != 5:
        raise RuntimeError("%s: series is [S + 1, B, steps, P, 3], got %s" % (name, tuple(series.shape)))
    R, B, steps, Ps, three = series.shape
    HW = Hh * Ww
    if Cc != 3 or Ps != P or three != 3 or kB != k * B or tuple(a.shape) != (B, 3) or (m is not None and tuple(m.shape) != (B, 3, HW)):
        raise RuntimeError("%s: series %s, m %s, a %s do not fit %d rows of %s and %d probes" % (
            name, tuple(series.shape), None if m is None else tuple(m.shape), tuple(a.shape), k, tuple(y.shape), P))
    if not (series.is_contiguous() and a.is_contiguous() and (m is None or (m.is_contiguous() and m.is_cuda and m.dtype == torch.float32))):
        raise RuntimeError("%s: contiguous fp32 device tables" % name)
    return ptr, ps, co, R, B, Hh, Ww, steps


def ens_corr_probe(y, a, m, series, probes, pairs, lags, k, row0, t):
    """Write the fluctuations of one chunk of k rows (y: NHWC [k*B, H, W, 3] or a channel-slice view, rows member-major) at the probe
    pixels into series [S + 1, B, steps, P, 3] at the timed step t, rows row0 .. row0 + k - 1 (the target: k = 1, row0 = S), about the
    mean planes m [B, 3, HW] (None: 0) with the scales a [B, 3] (device fp32) (tmg_ens_corr_probe).  Before ens_corr_accum, on the
    same stream."""
    ptr, ps, co, R, B, Hh, Ww, steps = _corr_feed("ens_corr_probe", y, a, m, series, k, len(probes))
    _chk(lib().tmg_ens_corr_probe(c_vp(ptr), _i64(ps, co), _ptr(a), _ptr(m), _ptr(series), ens_corr_cfg(probes, pairs, lags),
                                  _i64(k, R - 1, B, Hh, Ww, row0, t, steps), _stream()), "tmg_ens_corr_probe")


def ens_corr_accum(y, a, m, series, raw, probes, pairs, lags, k, row0, t):
    """Add one chunk of k rows (y as in ens_corr_probe, which has written these rows' series at step t) to the live planes of the rows
    row0 .. row0 + k - 1 of the state raw [S + 1, B, P Q L + 2 |J| L, HW]: the planes of the lags tau_l <= t, stored instead of added
    at t == tau_l (tmg_ens_corr_accum)."""
    ptr, ps, co, R, B, Hh, Ww, steps = _corr_feed("ens_corr_accum", y, a, m, series, k, len(probes))
    check_act(raw)
    check_device(raw)
    npl = len(probes) * len(pairs) * len(lags) + 2 * len(set(cc[1] for cc in pairs)) * len(lags)
    if tuple(raw.shape) != (R, B, npl, Hh * Ww) or not raw.is_contiguous():
        raise RuntimeError("ens_corr_accum: raw is %s, not a contiguous %s" % (tuple(raw.shape), (R, B, npl, Hh * Ww)))
    _chk(lib().tmg_ens_corr_accum(c_vp(ptr), _i64(ps, co), _ptr(a), _ptr(m), _ptr(series), _ptr(raw), ens_corr_cfg(probes, pairs, lags),
                                  _i64(k, R - 1, B, Hh, Ww, row0, t, steps), _stream()), "tmg_ens_corr_accum")


def ens_corr_finalize(raw, pm, pv, outs, member_rho, lines, probes, pairs, lags, Hh, Ww, T):
    """The covariance and the Pearson coefficient of every row of the state raw [S + 1, B, NPL, HW] after T timed steps: outs =
    (cov_mean, cov_std, rho_mean, rho_std, target_cov, target_rho) [B, P, Q, L, HW] fp32, member_rho [B, S, P, Q, L, HW] or None,
    lines = (line_x [B, S + 1, P, Q, L, W], line_y [B, S + 1, P, Q, L, H]); pm, pv [S + 1, B, P, Q, L] fp64 on the device, the mean
    and the population variance of the probe's first n_l values (tmg_ens_corr_finalize)."""
    check_act(raw)
    check_device(raw)
    P, Q, L = len(probes), len(pairs), len(lags)
    npl = P * Q * L + 2 * len(set(cc[1] for cc in pairs)) * L
    if raw.dim() != 4 or raw.shape[2] != npl or raw.shape[3] != Hh * Ww or not raw.is_contiguous() or len(outs) != 6 or len(lines) != 2:
        raise RuntimeError("ens_corr_finalize: raw is [S + 1, B, %d, %d] fp32 on the device, got %s" % (npl, Hh * Ww, tuple(raw.shape)))
    R, B, _, HW = raw.shape
    for t in (pm, pv):
        if tuple(t.shape) != (R, B, P, Q, L) or t.dtype != torch.float64 or not (t.is_cuda and t.is_contiguous()):
            raise RuntimeError("ens_corr_finalize: pm and pv are [S + 1, B, P, Q, L] fp64 on the device, got %s" % (tuple(t.shape),))
    want = [(B, P, Q, L, HW)] * 6 + [(B, R, P, Q, L, Ww), (B, R, P, Q, L, Hh)]
    if member_rho is not None:
        want.append((B, R - 1, P, Q, L, HW))
    for t, shp in zip(list(outs) + list(lines) + ([member_rho] if member_rho is not None else []), want):
        check_act(t)
        if tuple(t.shape) != shp or not t.is_contiguous():
            raise RuntimeError("ens_corr_finalize: an output is %s, not a contiguous %s" % (tuple(t.shape), shp))
    _chk(lib().tmg_ens_corr_finalize(_ptr(raw), _ptr(pm), _ptr(pv), *[_ptr(t) for t in outs], _ptr(member_rho), _ptr(lines[0]),
                                     _ptr(lines[1]), ens_corr_cfg(probes, pairs, lags), _i64(R - 1, B, Hh, Ww, T), _stream()),
         "tmg_ens_corr_finalize")


def ens_spod_plan(S, B, Cg, HW, NB, acc=None):
    """The launch plan of ens_spod_csd / ens_spod_modes for S members (R = S + 1 rows with the target) of B cases, Cg selected channels
    of HW pixels and NB bins (tmg_ens_spod_plan; nothing is launched) -> dict: P pixel slices of SL pixels, L the fmaf terms of one
    partial (L P >= Cg HW), NT row macro-tiles of 64 rows over the 2 R rows of Z, pairs = the NT (NT + 1) / 2 macro-tile pairs (I, J),
    I <= J, in workspace order, part the floats of one partial, ws the workspace floats, vec whether the rows are read with 16-byte
    loads (HW a multiple of 4 and, when the accumulator acc or its address is given, a 16-byte aligned base), MB the pixel blocks of the
    modes kernel."""
    addr = 0 if acc is None else (int(acc) if isinstance(acc, int) else acc.data_ptr())
    plan = (c_i64 * 9)()
    _chk(lib().tmg_ens_spod_plan(_i64(S, B, Cg, HW, NB, addr & 15), plan), "tmg_ens_spod_plan")
    P, L, NP, ws, SL, NT, part, vec, MB = [int(v) for v in plan]
    pairs = [(i, j) for i in range(NT) for j in range(i, NT)]
    assert len(pairs) == NP
    return {"P": P, "L": L, "pairs": pairs, "ws": ws, "SL": SL, "NT": NT, "part": part, "vec": bool(vec), "MB": MB}


def ens_spod_csd(acc, cst, bins, channels, ws, csd_raw, Tn):
    """The cross-spectral density sums of the R rows of the temporal-spectrum accumulator acc [2 NF + 1, R, B, C, HW] (cst [3, NF]: its
    constants; Tn its window) at the selected bins and over the selected channels into csd_raw [B, NB, 2, R, R]:
    raw0 + i raw1 = sum conj(X_m) X_n; ws: the workspace (>= ens_spod_plan's floats) (tmg_ens_spod_csd)."""
    check_act(acc)
    check_device(acc)
    _, R, B, Cc, HW = acc.shape
    NF = cst.shape[1]
    if acc.shape[0] != 2 * NF + 1 or tuple(cst.shape) != (3, NF) or not acc.is_contiguous() or not cst.is_contiguous() or \
            tuple(csd_raw.shape) != (B, len(bins), 2, R, R) or not csd_raw.is_contiguous() or csd_raw.dtype != torch.float32:
        raise ValueError("ens_spod_csd: acc is [2 NF + 1, R, B, C, HW], cst [3, NF] and csd_raw [B, NB, 2, R, R] float32, got %s, %s and %s"
                         % (tuple(acc.shape), tuple(cst.shape), tuple(csd_raw.shape)))
    _chk(lib().tmg_ens_spod_csd(_ptr(acc), _ptr(cst), _i64(*bins), _i64(*channels), _ptr(ws), _ptr(csd_raw),
                                _i64(R - 1, B, Cc, HW, NF, Tn, len(bins), len(channels), ws.numel()), _stream()), "tmg_ens_spod_csd")


def ens_spod_modes(acc, cst, bins, channels, w, modes, Tn):
    """modes [B, NB, 2 J, Cg, HW] = w [B, NB, 16, 2 SP] (SP = S rounded up to 4) times the rows [Re X_0 .. Re X_{S-1}, 0 ..; Im X_0 ..
    Im X_{S-1}, 0 ..] of the accumulator acc [2 NF + 1, S + 1, B, C, HW] at the selected bins and channels (tmg_ens_spod_modes)."""
    check_act(acc)
    check_device(acc)
    _, R, B, Cc, HW = acc.shape
    NF = cst.shape[1]
    SP = (R - 1 + 3) // 4 * 4
    if acc.shape[0] != 2 * NF + 1 or tuple(cst.shape) != (3, NF) or not acc.is_contiguous() or not cst.is_contiguous():
        raise ValueError("ens_spod_modes: acc is [2 NF + 1, R, B, C, HW] and cst [3, NF], got %s and %s" % (tuple(acc.shape), tuple(cst.shape)))
    if w.dtype != torch.float32 or modes.dtype != torch.float32:
        raise ValueError("ens_spod_modes: w and modes are float32")
    if tuple(w.shape) != (B, len(bins), 16, 2 * SP) or not w.is_contiguous() or tuple(modes.shape[:2]) != (B, len(bins)) or \
            tuple(modes.shape[3:]) != (len(channels), HW) or modes.shape[2] % 2 or not modes.is_contiguous():
        raise ValueError("ens_spod_modes: w is [B, NB, 16, %d] and modes [B, NB, 2 J, Cg, HW], got %s and %s"
                         % (2 * SP, tuple(w.shape), tuple(modes.shape)))
    _chk(lib().tmg_ens_spod_modes(_ptr(acc), _ptr(cst), _i64(*bins), _i64(*channels), _ptr(w), _ptr(modes),
                                  _i64(R - 1, B, Cc, HW, NF, Tn, len(bins), len(channels), modes.shape[2] // 2), _stream()),
         "tmg_ens_spod_modes")


def spec_rows(y, u, out_mu, out_std, ft_w, yw, k):
    """Row transform of a chunk of k members (y: NHWC [k*B, H, W, C] or a channel-slice view; channels 0 and 1 un-normalised on
    load) into the planar workspace yw [2, k*B, H, W]; ft_w: the operand matrix [2, W, W] (tmg_spec_rows)."""
    kB, Hh, Ww, Cc = y.shape
    ptr, ps, co, _ = seg(y)
    _chk(lib().tmg_spec_rows(c_vp(ptr), _i64(ps, co), _ptr(u), _ptr(out_mu), _ptr(out_std), _ptr(ft_w), _ptr(yw),
                             _i64(k, kB // k, Hh, Ww, Cc, yw.numel()), _stream()), "tmg_spec_rows")


def spec_cols(ft_h, yw, perm, offs, part, n, Hh, Ww, NK):
    """Column transform of the n images in yw (ft_h: [2, H, H]) and the shell sums of every 16-column tile, in the order of the
    tiles' shell lists (perm, offs), into part [n, W/16, NK] (tmg_spec_cols)."""
    _chk(lib().tmg_spec_cols(_ptr(ft_h), _ptr(yw), _ptr(perm), _ptr(offs), _ptr(part), _i64(n, Hh, Ww, NK, yw.numel(), part.numel()),
                             _flts([0.5 / (float(Hh) * float(Ww)) ** 2]), _stream()), "tmg_spec_cols")


def spec_accum(part, smean, sm2, tmean, outs, ostride, k, B, NK, QT, n_before, m0, t_before, flags):
    """Fold the k members' spectra (part of spec_transform) into the step state (smean, sm2) or, flags & 2, write (spec_mean, spec_std)
    = `outs` with per-case stride ostride; flags & 1 advances the members' running time means tmean (tmg_spec_accum)."""
    outs = outs if outs is not None else (None,) * 2
    _chk(lib().tmg_spec_accum(_ptr(part), _ptr(smean), _ptr(sm2), _ptr(tmean), *[_ptr(t) for t in outs],
                              _i64(k, B, NK, QT, n_before, m0, t_before, flags, ostride), _stream()), "tmg_spec_accum")


def spec_finalize(tmean, tm_mean, tm_std, S, B, NK):
    """Mean / population std over the S members of their time-mean spectra (tmg_spec_finalize)."""
    _chk(lib().tmg_spec_finalize(_ptr(tmean), _ptr(tm_mean), _ptr(tm_std), _i64(S, B, NK), _stream()), "tmg_spec_finalize")


def tspec_store(y, u, out_mu, out_std, ring, k, m0, slot):
    """Un-normalise one chunk of k members (y: NHWC [k*B, H, W, C] or a channel-slice view, rows member-major) into rows m0 .. m0 + k - 1
    of slot `slot` of the planar ring [16, S, B, C, HW] (tmg_tspec_store)."""
    kB, Hh, Ww, Cc = y.shape
    ptr, ps, co, _ = seg(y)
    _chk(lib().tmg_tspec_store(c_vp(ptr), _i64(ps, co), _ptr(u), _ptr(out_mu), _ptr(out_std), _ptr(ring),
                               _i64(k, kB // k, Hh * Ww, Cc, ring.shape[1], m0, slot), _stream()), "tmg_tspec_store")


def tspec_block(tm, ring, acc, Tn, NF, n0, nb, first):
    """Fold the nb <= 16 valid slots of ring [16, S, B, C, HW], which hold steps n0 .. n0 + nb - 1, into acc [2 NF + 1, S, B, C, HW] with
    rows n0 .. n0 + nb - 1 of the operand tm [Tn, RP]; first: acc is written, else added to (tmg_tspec_block)."""
    _chk(lib().tmg_tspec_block(_ptr(tm), _ptr(ring), _ptr(acc), _i64(ring[0].numel(), Tn, NF, n0, nb, 1 if first else 0), _stream()),
         "tmg_tspec_block")


def tspec_finalize(acc, cst, psd_mean, psd_std, S, B, C, HW, NF, Tn):
    """P_k of every member from acc and the constants cst [3, NF] = (Re G_k, Im G_k, c_k / Tn^2), then mean / population std over the S
    members into psd_mean / psd_std [B, NF, C, H, W] (tmg_tspec_finalize)."""
    _chk(lib().tmg_tspec_finalize(_ptr(acc), _ptr(cst), _ptr(psd_mean), _ptr(psd_std), _i64(S, B, C, HW, NF), _flts([1.0 / float(Tn)]),
                                  _stream()), "tmg_tspec_finalize")


def reverse_loss_fwd(y, ld, loss, s1, s2):
    _chk(lib().tmg_reverse_loss_fwd(_ptr(y), _ptr(ld), _ptr(loss), _i64(y.numel(), ld.numel()), _flts([s1, s2]), _stream()), "tmg_reverse_loss_fwd")


def reverse_loss_bwd(y, g, dy, dld, s1, s2):
    _chk(lib().tmg_reverse_loss_bwd(_ptr(y), _ptr(g), _ptr(dy), _ptr(dld), _i64(y.numel(), dld.numel()), _flts([s1, s2]), _stream()), "tmg_reverse_loss_bwd")


SUM_TERMS_MAX = 8


def sum_terms(terms, out):
    """out[b] = sum of the terms (fp32 vectors of out's length, or one-element tensors: broadcast) in one launch (tmg_sum_terms)."""
    n = len(terms)
    ptrs = (c_vp * n)(*[t.data_ptr() for t in terms])
    _chk(lib().tmg_sum_terms(ptrs, _i64(*[t.numel() for t in terms]), c_i64(n), _ptr(out), c_i64(out.numel()), _stream()), "tmg_sum_terms")


def vec_sum(g, out):
    _chk(lib().tmg_vec_sum(_ptr(g), c_i64(g.numel()), _ptr(out), _stream()), "tmg_vec_sum")


def spread2(dy, up):
    """up (contiguous [B,H,W,C]) = dy on the even positions, zeros elsewhere, in one launch (tmg_spread2); False outside the envelope."""
    B, Hh, Ww, C = up.shape
    rc = lib().tmg_spread2(_ptr(dy), _d2(dy), _ptr(up), _i64(B, Hh, Ww, dy.shape[1], dy.shape[2], C), _stream())
    return _launched(rc, "tmg_spread2")


def level_pack(tab, Wz, Wcat, Bz, Kp, NL, NLp, C, ch, Cc):
    """Stacked / sliced parameter operands of a level node from the modules' own tensors (tmg_level_pack; tab from _segment_table)."""
    _chk(lib().tmg_level_pack(_ptr(tab), _ptr(Wz), _ptr(Wcat), _ptr(Bz), _ptr(Kp), _i64(NL, NLp, C, ch, Cc), _stream()), "tmg_level_pack")


def checker(src, dst, to_small):
    if to_small:
        B, h, w, _ = dst.shape
        C = src.shape[3]
    else:
        B, h, w, _ = src.shape
        C = dst.shape[3]
    _chk(lib().tmg_checker(_ptr(src), _d2(src), _ptr(dst), _d2(dst), _i64(B, h, w, C, to_small), _stream()), "tmg_checker")


def pad_halves(src, dst, ch, pad, to_padded):
    """compact [B,H,W,2 ch] <-> zero-padded [B,H,W,2 (ch + pad)] = [x1 | 0.. | x2 | 0..] (one launch, zeros included)."""
    B, Hh, Ww, _ = src.shape
    assert src.shape[3] == (2 * ch if to_padded else 2 * (ch + pad)) and dst.shape[3] == (2 * (ch + pad) if to_padded else 2 * ch)
    _chk(lib().tmg_pad_halves(_ptr(src), _d2(src), _ptr(dst), _d2(dst), _i64(B * Hh * Ww, ch, pad, 1 if to_padded else 0), _stream()),
         "tmg_pad_halves")


def upsample_fwd(src, dst):
    B, hi, wi, C = src.shape
    _, ho, wo, _ = dst.shape
    assert src.is_contiguous() and dst.is_contiguous()
    _chk(lib().tmg_upsample_fwd(_ptr(src), _ptr(dst), _i64(B, hi, wi, ho, wo, C), _stream()), "tmg_upsample_fwd")


def upsample_bwd(dout, din):
    B, hi, wi, C = din.shape
    _, ho, wo, _ = dout.shape
    assert dout.is_contiguous() and din.is_contiguous()
    _chk(lib().tmg_upsample_bwd(_ptr(dout), _ptr(din), _i64(B, hi, wi, ho, wo, C), _stream()), "tmg_upsample_bwd")


def chan_reduce(x, g, v0, v1, v2, v3, s0, s1, mode, divisor=0):
    """mode 0 with divisor > 0: v0 holds channel SUMS and v0/divisor is subtracted (centred second pass)."""
    B, H, W, C = x.shape
    _chk(lib().tmg_chan_reduce(_ptr(x), _d2(x), _ptr(g), _d2(g), _ptr(v0), _ptr(v1), _ptr(v2), _ptr(v3), _ptr(s0), _ptr(s1),
                               _i64(B * H * W, C, mode, divisor), _stream()), "tmg_chan_reduce")


def bn_bwd_apply(x, g, a, bsh, mean, rstd, gamma, m0, m1, dx, accumulate, divisor=0):
    """divisor > 0: m0, m1 are sums and are divided by it inside the kernel.  m0 = m1 = None: the statistics are constants (eval mode)."""
    B, H, W, C = x.shape
    assert (m0 is None) == (m1 is None)
    _chk(lib().tmg_bn_bwd_apply(_ptr(x), _d2(x), _ptr(g), _d2(g), _ptr(a), _ptr(bsh), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(m0),
                                _ptr(m1), _ptr(dx), _d2(dx), _i64(B * H * W, C, accumulate, divisor), _stream()), "tmg_bn_bwd_apply")


def chan_moments(x, acc64):
    """One-pass per-channel sum / sum of squares of an NHWC tensor or channel-slice view into acc64 (double [2, C], zeroed)."""
    B, H, W, C = x.shape
    assert acc64.dtype == torch.float64 and acc64.numel() == 2 * C
    _chk(lib().tmg_chan_moments(_ptr(x), _d2(x), _ptr(acc64), _i64(B * H * W, C), _stream()), "tmg_chan_moments")


def bn_finalize64(acc64, gamma, beta, running_mean, running_var, out, n, eps, momentum, counter=None):
    """counter: the module's int64 num_batches_tracked tensor (device scalar), incremented by the same launch."""
    C = gamma.numel()
    if counter is not None:
        assert counter.dtype == torch.int64 and counter.numel() == 1 and counter.device == gamma.device
    _chk(lib().tmg_bn_finalize64(_ptr(acc64), _ptr(gamma), _ptr(beta), _ptr(running_mean), _ptr(running_var), _ptr(out),
                                 _i64(C, n, counter.data_ptr() if counter is not None else 0), _flts([eps, momentum]), _stream()),
         "tmg_bn_finalize64")


def bn_finalize(sums, csq, gamma, beta, running_mean, running_var, out, n, eps, momentum):
    """out: [5, C] = mean, var, rstd, a, bsh; running_* (or None) updated in place."""
    C = gamma.numel()
    _chk(lib().tmg_bn_finalize(_ptr(sums), _ptr(csq), _ptr(gamma), _ptr(beta), _ptr(running_mean), _ptr(running_var), _ptr(out), _i64(C, n),
                               _flts([eps, momentum]), _stream()), "tmg_bn_finalize")


def masked_add(dst, src=None, ref=None, add=None, accumulate=False):
    B, H, W, n = dst.shape
    _chk(lib().tmg_masked_add(_ptr(src), _d2(src), _ptr(ref), _d2(ref), _ptr(add), _d2(add), _ptr(dst), _d2(dst),
                              _i64(B * H * W, n, accumulate), _stream()), "tmg_masked_add")


def c1_fwd(inputs, w, out, relu_in=True, w_rows=0, fill4=False, add=None, w_split=0, w_gap=0):
    B, H, W, _ = inputs[0].shape
    ip, idesc, n_in = _segs(inputs)
    Cin = sum(t.shape[3] for t in inputs)
    _chk(lib().tmg_c1_fwd_add(ip, idesc, c_i64(n_in), _ptr(w), _ptr(add), _d2(add), _ptr(out), _d2(out),
                              _i64(B, H, W, Cin, relu_in, w_rows, fill4, w_split, w_gap), _stream()), "tmg_c1_fwd_add")


def c1x2_fwd(inputs, w1, w2, out, w_rows, w2_d1_row, add1=None, add2=None, w_split=0, w_gap=0, relu_in=True):
    """Both growth-1 layers in one launch; out: [B,H,W,4] receives (d1, d2, 0, 0)."""
    B, H, W, _ = inputs[0].shape
    ip, idesc, n_in = _segs(inputs)
    Cin = sum(t.shape[3] for t in inputs)
    _chk(lib().tmg_c1x2_fwd(ip, idesc, c_i64(n_in), _ptr(w1), _ptr(w2), _ptr(add1), _d2(add1), _ptr(add2), _d2(add2), _ptr(out), _d2(out),
                            _i64(B, H, W, Cin, relu_in, w_rows, w_split, w_gap, w2_d1_row), _stream()), "tmg_c1x2_fwd")


def c1_bwd(inputs, w, dW, dd, dref, gsegs, relu_in=True):
    B, H, W, _ = inputs[0].shape
    ip, idesc, n_in = _segs(inputs)
    gp, gdesc, ng = _segs(gsegs)
    Cin = sum(t.shape[3] for t in inputs)
    _chk(lib().tmg_c1_bwd(ip, idesc, c_i64(n_in), _ptr(w), _ptr(dW), _ptr(dd), _d2(dd), _ptr(dref), _d2(dref), gp, gdesc, c_i64(ng),
                          _i64(B, H, W, Cin, relu_in), _stream()), "tmg_c1_bwd")


def dkappa(w, dw, b, db, kappa, dk):
    """dk += <w, dw> + <b, db> when kappa lies inside its clamp range (b / db None: a convolution without bias)."""
    _chk(lib().tmg_dkappa(_ptr(w), _ptr(dw), c_i64(w.numel()), _ptr(b), _ptr(db), c_i64(b.numel() if b is not None else 0), _ptr(kappa),
                          _ptr(dk), _stream()),
         "tmg_dkappa")


def dense2_bwd(inputs, w1p, w2p, dW1p, dW2p, GD, D, g0, outs, cin_nn, add0=None, rows1=0, rows2=0, dd1=None, dd2=None, split2=0, gap2=0,
               dd_quad=False, g0_masked=False):
    """Fused backward of the two growth-1 layers; `inputs` = nn inputs + [D]; g0 / outs: lists (<= 2) of NHWC tensors.
    g0_masked: g0 / GD come from coupling_bwd's summed form (g0 may be the output tensor itself; add0 must be None)."""
    B, H, W, _ = inputs[0].shape
    ip, idesc, n_in = _segs(inputs)
    gp, gdesc, ng = _segs(g0)
    op, odesc, _ = _segs(outs)
    Cin = sum(t.shape[3] for t in inputs)
    a_stride = seg(add0)[1] if add0 is not None else 0
    _chk(lib().tmg_dense2_bwd(ip, idesc, c_i64(n_in), _ptr(w1p), _ptr(w2p), _ptr(dW1p), _ptr(dW2p), _ptr(GD), c_i64(seg(GD)[1]), _ptr(D),
                              c_i64(seg(D)[1]), gp, gdesc, op, odesc, c_i64(ng), _ptr(add0), c_i64(a_stride),
                              _i64(B, H, W, Cin, cin_nn, rows1 or Cin, rows2 or Cin, dd1.data_ptr() if dd1 is not None else 0,
                                   dd2.data_ptr() if dd2 is not None else 0, seg(dd1)[1] if dd1 is not None else 0, split2, gap2, 1 if dd_quad else 0,
                                   1 if g0_masked else 0),
                              _stream()),
         "tmg_dense2_bwd")


# ------------------------------------------------------------------------------------------------
# physics-constrained loss (row F1)
# ------------------------------------------------------------------------------------------------
def phys_fields(u, p, ustar, pstar, dx, dy, rho, k1, k2, scale):
    """Divergence / pressure-Poisson residual fields for 3x3 or 5x5 stencils, scaled or not (tmg_phys_fields).  u: contiguous
    [N,2,H,W]; p: contiguous [N,1,H,W] or None; ustar [N,1,H,W+2] / pstar [N,1,H,W] (either may be None)."""
    check_act(u)
    N, _, Hh, Ww = u.shape
    rc = lib().tmg_phys_fields(_ptr(u), _ptr(p), _ptr(ustar), _ptr(pstar), _i64(N, Hh, Ww, k1, k2, 1 if scale else 0), _flts([dx, dy, rho]), _stream())
    if rc == -100:
        raise ValueError('kernel_size size {:d} is not supported!'.format(k1 if k1 not in (3, 5) else k2))
    _chk(rc, "tmg_phys_fields")


def phys_fields_bwd(u, p, gustar, gpstar, du, dp, dx, dy, rho, k1, k2, scale):
    """Adjoint of phys_fields (tmg_phys_fields_bwd): du [N,2,H,W] and dp [N,1,H,W] (or None) are overwritten with the gradient of
    sum(gustar * ustar) + sum(gpstar * pstar).  u / p as for phys_fields (p may be None when gpstar is None); gustar [N,1,H,W+2] /
    gpstar [N,1,H,W], contiguous, either may be None."""
    check_act(u)
    N, _, Hh, Ww = u.shape
    rc = lib().tmg_phys_fields_bwd(_ptr(u), _ptr(p), _ptr(gustar), _ptr(gpstar), _ptr(du), _ptr(dp), _i64(N, Hh, Ww, k1, k2, 1 if scale else 0),
                                   _flts([dx, dy, rho]), _stream())
    if rc == -100:
        raise ValueError('kernel_size size {:d} is not supported!'.format(k1 if k1 not in (3, 5) else k2))
    _chk(rc, "tmg_phys_fields_bwd")


def phys_fwd(y, target, sums, sd, mu, dx, dy, rho=1.0, pstar=None, ustar=None):
    """y / target: contiguous [N,3,H,W]; sums: zero-filled [3] (sum pstar^2, sum ustar^2, sum (y-target)^2)."""
    check_act(y)
    N, _, Hh, Ww = y.shape
    _chk(lib().tmg_phys_fwd(_ptr(y), _ptr(target), _ptr(sums), _ptr(pstar), _ptr(ustar), _i64(N, Hh, Ww),
                            _flts(list(sd) + list(mu) + [dx, dy, rho]), _stream()), "tmg_phys_fwd")


def phys_rms(y, trms, mean_out, coef_out, sum_out):
    """y: contiguous [B,T,3,H,W]; trms: [B,3,H,W]; sum_out: zero-filled [1]."""
    B, T = y.shape[0], y.shape[1]
    chw = y.shape[2] * y.shape[3] * y.shape[4]
    _chk(lib().tmg_phys_rms(_ptr(y), _ptr(trms), _ptr(mean_out), _ptr(coef_out), _ptr(sum_out), _i64(B, T, chw), _stream()), "tmg_phys_rms")


def phys_bwd(y, target, mean, coef, dyo, T, sd, mu, dx, dy, rho, cp, cd, cl, cr, upstream=None):
    """upstream: optional device scalar (fp32, 1 element) multiplied onto cp..cr inside the kernel."""
    N, _, Hh, Ww = y.shape
    _chk(lib().tmg_phys_bwd_dev(_ptr(y), _ptr(target), _ptr(mean), _ptr(coef), _ptr(dyo), _ptr(upstream), _i64(N, T, Hh, Ww),
                                _flts(list(sd) + list(mu) + [dx, dy, rho, cp, cd, cl, cr]), _stream()), "tmg_phys_bwd_dev")
