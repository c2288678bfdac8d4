// The physical value of a normalised channel and the 3x3 first-derivative stencil on it: what the ensemble diagnostics that must agree
// bit for bit share.  A header, compiled into each user with that file's own flags.  Every function rounds each operation on its own
// (contraction is off inside it, whatever its caller's setting), so a caller gets the same bits from the same operands in every file.
//
// The physical value.  TWO definitions, which give different bits and stay two:
//   tmg_unnorm_fma    fl(sc fma(sd, x, mu))        the ensemble statistics' yh (tmg_ensemble.hip) and everything that continues it: the
//                                                  vorticity of ens_turb_accum_kernel, the fields of the spectra (spec_rows_kernel,
//                                                  tspec_store_kernel, xspec_prep_kernel) and the prediction intervals
//                                                  (ens_quant_step_kernel)
//   tmg_unnorm_split  fl(sc fl(fl(sd x) + mu))     the derived fields of the pooled PDFs (ens_pdf_count_kernel) and the vortex census
//                                                  (ens_vortex_classify_kernel): the tests' numpy float32 mirror has no fma
//
// The stencil.  tmg_sx<FMA> / tmg_sy<FMA>: 8 dx d/dx and 8 dy d/dy of the physical value of channel c under zero padding, FMA choosing
// the definition above.  The taps are added one by one onto 0 in a fixed order:
//   Sx   the right column, then the left one (subtracted), each as centre times 2, up, down
//   Sy   the lower row, then the upper one (subtracted), each as centre times 2, left, right
// ens_pdf_count_kernel's vort and ens_vortex_classify_kernel's omega are the same function of the same operands: equal by construction.
// With FMA the doubled tap is one fma onto the running sum, as ens_turb_accum_kernel has always been compiled; 2 v is exact, so the
// value is that of the separate product and sum (unless 2 v overflows where the sum does not).
//
// tmg_sobel3: the same 1, 2, 1 combination of three differences that the caller has formed, fl(fl(d0 + fl(2 d1)) + d2): Sx with d_i the
// column difference of row h - 1 + i, Sy with d_i the row difference of column w - 1 + i
//   Sx f = fl(fl(fl(f[h-1,w+1] - f[h-1,w-1]) + fl(2 fl(f[h,w+1] - f[h,w-1]))) + fl(f[h+1,w+1] - f[h+1,w-1]))
//   Sy f = the same with the roles of h and w exchanged (row h + 1 minus row h - 1)
// ens_budget_accum_kernel (tmg_budget.hip, f the fluctuations) calls it.  ens_flux_accum_kernel (tmg_flux.hip, f the box sums) writes
// the same expression out in its kernel: behind this function two of its packed additions came out with their operands exchanged,
// and the kernel alone then took 0.5071 ms in the median of three runs against 0.5051 ms, outside the 0.5042 .. 0.5058 ms that the
// unchanged kernel spanned in the same session.  Their float32 host mirrors follow this order.
#pragma once
#include "tmg_common.h"

static __device__ __forceinline__ float tmg_unnorm_fma(float x, float sc, float sd, float mu) {
    // One fma, then one multiply whose ROUNDED product is the value.  Contraction is off so that the multiply is never fused into a
    // later subtraction (yh - mean would then see the unrounded product, and a member that is constant in time would leave a
    // co-moment of rounding size instead of exactly 0).
#pragma clang fp contract(off)
    const float t = __builtin_fmaf(sd, x, mu);
    return sc * t;
}

static __device__ __forceinline__ float tmg_unnorm_split(float x, float sc, float sd, float mu) {
#pragma clang fp contract(off)
    float t = sd * x;
    t = t + mu;
    return sc * t;
}

template <bool FMA>
static __device__ __forceinline__ float tmg_unnorm(float x, float sc, float sd, float mu) {
    return FMA ? tmg_unnorm_fma(x, sc, sd, mu) : tmg_unnorm_split(x, sc, sd, mu);
}

// yp: the pixel's channel 0; ps, rs: floats to the next pixel and to the next row; up, dn, lf, rt: whether that neighbour is in the field
template <bool FMA>
static __device__ __forceinline__ float tmg_sx(const float* __restrict__ yp, long long ps, long long rs, int c, float sc, float sd,
                                               float mu, bool up, bool dn, bool lf, bool rt) {
#pragma clang fp contract(off)
    float a = 0.f;
    if (rt) {
        const float v = tmg_unnorm<FMA>((yp + ps)[c], sc, sd, mu);
        a = FMA ? __builtin_fmaf(2.f, v, a) : a + 2.f * v;
        if (up) a += tmg_unnorm<FMA>((yp + ps - rs)[c], sc, sd, mu);
        if (dn) a += tmg_unnorm<FMA>((yp + ps + rs)[c], sc, sd, mu);
    }
    if (lf) {
        const float v = tmg_unnorm<FMA>((yp - ps)[c], sc, sd, mu);
        a = FMA ? __builtin_fmaf(-2.f, v, a) : a - 2.f * v;
        if (up) a -= tmg_unnorm<FMA>((yp - ps - rs)[c], sc, sd, mu);
        if (dn) a -= tmg_unnorm<FMA>((yp - ps + rs)[c], sc, sd, mu);
    }
    return a;
}

template <bool FMA>
static __device__ __forceinline__ float tmg_sy(const float* __restrict__ yp, long long ps, long long rs, int c, float sc, float sd,
                                               float mu, bool up, bool dn, bool lf, bool rt) {
#pragma clang fp contract(off)
    float a = 0.f;
    if (dn) {
        const float v = tmg_unnorm<FMA>((yp + rs)[c], sc, sd, mu);
        a = FMA ? __builtin_fmaf(2.f, v, a) : a + 2.f * v;
        if (lf) a += tmg_unnorm<FMA>((yp + rs - ps)[c], sc, sd, mu);
        if (rt) a += tmg_unnorm<FMA>((yp + rs + ps)[c], sc, sd, mu);
    }
    if (up) {
        const float v = tmg_unnorm<FMA>((yp - rs)[c], sc, sd, mu);
        a = FMA ? __builtin_fmaf(-2.f, v, a) : a - 2.f * v;
        if (lf) a -= tmg_unnorm<FMA>((yp - rs - ps)[c], sc, sd, mu);
        if (rt) a -= tmg_unnorm<FMA>((yp - rs + ps)[c], sc, sd, mu);
    }
    return a;
}

static __device__ __forceinline__ float tmg_sobel3(float d0, float d1, float d2) {
#pragma clang fp contract(off)
    return (d0 + 2.f * d1) + d2;
}
