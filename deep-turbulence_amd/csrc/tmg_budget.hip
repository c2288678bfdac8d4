// The budget of the turbulent kinetic energy k = 1/2 <u'_i u'_i> of sampled roll-outs and of the target (tmg_ops.EnsembleBudget /
// utils.modelPredBudget): production, convection, turbulent transport, pressure diffusion, viscous diffusion and dissipation, from
// time sums of products of every row's own fluctuations.  Rows are the S members plus the target as row S.
//   ens_budget_accum_kernel<V>   one thread per pixel (V = 0) or per four consecutive pixels of one field row (V = 1) of a case; it
//                                loops over the chunk's k members and adds 14 quantities to the member's own planes of
//                                raw [S + 1][B][14][HW].  The order: with d_c = fl(a_c fl(y_c - m_c)), c = 0, 1, 2 (u, v, p; one
//                                subtraction, one multiplication), d = 0 outside the field, and Sx, Sy the tmg_sobel3 (tmg_field.h) of
//                                the three column / row differences of the fluctuation d_c, the planes are
//                                  0..2: d_u, d_v, d_p;  3..5: fl(d_u d_u), fl(d_u d_v), fl(d_v d_v);
//                                  6..9: fl(fl(d_u d_u) d_u), fl(fl(d_u d_u) d_v), fl(fl(d_u d_v) d_v), fl(fl(d_v d_v) d_v);
//                                  10, 11: fl(d_p d_u), fl(d_p d_v);
//                                  12: fl(fl(Sx d_u Sx d_u) + fl(Sx d_v Sx d_v));  13: the same with Sy
//                                and raw = fl(raw + term), one addition per timed step, in step order; the first timed step stores
//                                the term itself, so the state needs no memset.  Every operation is rounded on its own (no
//                                contraction): a float32 host mirror gives the same bits.
//                                An element of raw is touched by one thread once per step: no atomics, no LDS, no partial sums, so
//                                the state is bitwise reproducible and does not depend on the chunking.
//                                Stencil operands are direct neighbour loads, no LDS tile, for the reasons given above
//                                ens_turb_accum_kernel (tmg_ensemble.hip): the neighbours along W are the adjacent lanes' own pixels,
//                                the rows above and below are lines the neighbouring waves load anyway, and the NHWC input with its
//                                run-time pixel stride would fill a tile by the same strided loads.  The kernel is bound by its
//                                state: 14 planes read and written per member and step (112 bytes per pixel) against 12 bytes of
//                                input.  The plane accesses are coalesced along the pixels (one dword per lane, or one 16-byte
//                                vector per lane for V = 1), and all 14 loads of a member are issued before its arithmetic and
//                                the 14 stores come last, so that no store sits between two loads.
//   ens_budget_terms_kernel      once per mini-batch: one thread per (case, pixel) loops over the S + 1 rows; in fp64 it forms the
//                                central moments at the pixel and at its eight neighbours straight from raw (shift formulas, T the
//                                timed steps, D_c = raw_c / T), the seven terms, and a Welford mean / M2 over the members in member
//                                order.  No plane of intermediates is written.
#include "tmg_field.h"
#include "tmglow_hip.h"
#include "tmglow_hip_budget.h"

#define BUDGET_MAXS 1024
#define BUDGET_THREADS 256
#define BUDGET_Q 14

struct BudgetPlan {
    int64_t tile, tiles, vec;
};

// vec_ok: the base of raw is 16-byte aligned.  Four pixels per thread must lie in one field row: W % 4 == 0.
static BudgetPlan budget_plan(int64_t Hh, int64_t Ww, int vec_ok) {
    BudgetPlan g;
    const int64_t HW = Hh * Ww;
    g.vec = (vec_ok && Ww % 4 == 0) ? 1 : 0;
    g.tile = g.vec ? 4 * BUDGET_THREADS : BUDGET_THREADS;
    g.tiles = (HW + g.tile - 1) / g.tile;
    return g;
}

template <int V>
__global__ __launch_bounds__(BUDGET_THREADS) void ens_budget_accum_kernel(const float* __restrict__ y, int ps, const float* __restrict__ a,
                                                                          const float* __restrict__ m, float* __restrict__ raw, int k,
                                                                          int B, int Hh, int Ww, int row0, int first) {
#pragma clang fp contract(off)
    constexpr int PX = V ? 4 : 1, NW = PX + 2;                                 // the window: columns w - 1 .. w + PX of rows h - 1 .. h + 1
    const int HW = Hh * Ww;
    const long long p = ((long long)blockIdx.x * BUDGET_THREADS + threadIdx.x) * PX;
    const int b = blockIdx.y;
    if (p >= HW) return;                                                       // (V: W % 4 == 0, so p + 3 is in the same row)
    const int h = (int)(p / Ww), w = (int)(p - (long long)h * Ww);
    const size_t hw = (size_t)HW;
    const float a0 = a[b * 3], a1 = a[b * 3 + 1], a2 = a[b * 3 + 2];
    bool in[3][NW];
    long long off[3][NW];                                                      // pixel offset of the window's entries from p
    float m0[3][NW], m1[3][NW], m2[PX];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < NW; ++j) {
            const int hh = h + i - 1, ww = w + j - 1;
            in[i][j] = hh >= 0 && hh < Hh && ww >= 0 && ww < Ww;
            off[i][j] = (long long)(i - 1) * Ww + (j - 1);
            m0[i][j] = 0.f, m1[i][j] = 0.f;
            if (m && in[i][j]) {
                const float* mp = m + (size_t)b * 3 * hw + (size_t)(p + off[i][j]);
                m0[i][j] = mp[0];
                m1[i][j] = mp[hw];
            }
        }
    }
#pragma unroll
    for (int j = 0; j < PX; ++j) m2[j] = m ? m[((size_t)b * 3 + 2) * hw + (size_t)p + j] : 0.f;
    for (int s = 0; s < k; ++s) {
        float* rp = raw + ((size_t)(row0 + s) * B + b) * BUDGET_Q * hw + (size_t)p;
        float r[BUDGET_Q][PX];
        if (!first) {                                                          // uniform; all 14 loads first
#pragma unroll
            for (int q = 0; q < BUDGET_Q; ++q) {
                if constexpr (V) {
                    const float4 t = *reinterpret_cast<const float4*>(rp + q * hw);
                    r[q][0] = t.x, r[q][1] = t.y, r[q][2] = t.z, r[q][3] = t.w;
                } else {
                    r[q][0] = rp[q * hw];
                }
            }
        }
        const float* yp = y + ((size_t)((size_t)s * B + b) * hw + (size_t)p) * ps;
        float du[3][NW], dv[3][NW];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < NW; ++j) {
                du[i][j] = 0.f, dv[i][j] = 0.f;                                // a value outside the field counts as 0
                if (in[i][j]) {
                    const float* q = yp + off[i][j] * ps;
                    const float tu = q[0] - m0[i][j], tv = q[1] - m1[i][j];
                    du[i][j] = a0 * tu;
                    dv[i][j] = a1 * tv;
                }
            }
        }
        float t[BUDGET_Q][PX];
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            const float tp = yp[(size_t)j * ps + 2] - m2[j];
            const float u = du[1][j + 1], v = dv[1][j + 1], pr = a2 * tp;
            const float uu = u * u, uv = u * v, vv = v * v;
            t[0][j] = u, t[1][j] = v, t[2][j] = pr;
            t[3][j] = uu, t[4][j] = uv, t[5][j] = vv;
            t[6][j] = uu * u, t[7][j] = uu * v, t[8][j] = uv * v, t[9][j] = vv * v;
            t[10][j] = pr * u, t[11][j] = pr * v;
            // window column j + 1 is the pixel's own
            const float xu0 = du[0][j + 2] - du[0][j], xu1 = du[1][j + 2] - du[1][j], xu2 = du[2][j + 2] - du[2][j];
            const float xv0 = dv[0][j + 2] - dv[0][j], xv1 = dv[1][j + 2] - dv[1][j], xv2 = dv[2][j + 2] - dv[2][j];
            const float sxu = tmg_sobel3(xu0, xu1, xu2), sxv = tmg_sobel3(xv0, xv1, xv2);
            const float yu0 = du[2][j] - du[0][j], yu1 = du[2][j + 1] - du[0][j + 1], yu2 = du[2][j + 2] - du[0][j + 2];
            const float yv0 = dv[2][j] - dv[0][j], yv1 = dv[2][j + 1] - dv[0][j + 1], yv2 = dv[2][j + 2] - dv[0][j + 2];
            const float syu = tmg_sobel3(yu0, yu1, yu2), syv = tmg_sobel3(yv0, yv1, yv2);
            const float gxu = sxu * sxu, gxv = sxv * sxv, gyu = syu * syu, gyv = syv * syv;
            t[12][j] = gxu + gxv;
            t[13][j] = gyu + gyv;
        }
#pragma unroll
        for (int q = 0; q < BUDGET_Q; ++q) {
#pragma unroll
            for (int j = 0; j < PX; ++j) r[q][j] = first ? t[q][j] : r[q][j] + t[q][j];
        }
#pragma unroll
        for (int q = 0; q < BUDGET_Q; ++q) {                                   // all 14 stores last
            if constexpr (V) *reinterpret_cast<float4*>(rp + q * hw) = make_float4(r[q][0], r[q][1], r[q][2], r[q][3]);
            else rp[q * hw] = r[q][0];
        }
    }
}

// The central moments of one row at one pixel, fp64, straight from the raw sums (T = the timed steps).
struct BudgetMoments {
    double Du, Dv, Dp, uu, uv, vv, uuu, uuv, uvv, vvv, pu, pv;
};

__device__ __forceinline__ BudgetMoments budget_moments(const float* __restrict__ rp, size_t hw, double T) {
#pragma clang fp contract(off)
    BudgetMoments o;
    double e[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) e[q] = (double)rp[q * hw] / T;
    const double Du = e[0], Dv = e[1], Dp = e[2];
    o.Du = Du, o.Dv = Dv, o.Dp = Dp;
    o.uu = e[3] - Du * Du;
    o.uv = e[4] - Du * Dv;
    o.vv = e[5] - Dv * Dv;
    o.uuu = (e[6] - 3.0 * Du * e[3]) + 2.0 * Du * Du * Du;
    o.uuv = ((e[7] - 2.0 * Du * e[4]) - Dv * e[3]) + 2.0 * Du * Du * Dv;
    o.uvv = ((e[8] - 2.0 * Dv * e[4]) - Du * e[5]) + 2.0 * Du * Dv * Dv;
    o.vvv = (e[9] - 3.0 * Dv * e[5]) + 2.0 * Dv * Dv * Dv;
    o.pu = e[10] - Dp * Du;
    o.pv = e[11] - Dp * Dv;
    return o;
}

struct BudgetFl {
    double dx, dy, nu, rho;
};

__global__ __launch_bounds__(BUDGET_THREADS) void ens_budget_terms_kernel(const float* __restrict__ raw, const double* __restrict__ M,
                                                                          BudgetFl fl, float* __restrict__ bmean, float* __restrict__ bstd,
                                                                          float* __restrict__ tbud, float* __restrict__ smean,
                                                                          float* __restrict__ sstd, float* __restrict__ tstr,
                                                                          float* __restrict__ mbud, int S, int B, int Hh, int Ww, int Tn) {
#pragma clang fp contract(off)
    const int HW = Hh * Ww;
    const long long p = (long long)blockIdx.x * BUDGET_THREADS + threadIdx.x;
    const int b = blockIdx.y;
    if (p >= HW) return;
    const int h = (int)(p / Ww), w = (int)(p - (long long)h * Ww);
    const bool inner = h > 0 && h + 1 < Hh && w > 0 && w + 1 < Ww;
    const size_t hw = (size_t)HW;
    const double T = (double)Tn, ex = 8.0 * fl.dx, ey = 8.0 * fl.dy, dx2 = fl.dx * fl.dx, dy2 = fl.dy * fl.dy;
    const double nanv = __builtin_nan("");
    double mean[10], m2[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) mean[i] = 0.0, m2[i] = 0.0;
    for (int r = 0; r <= S; ++r) {
        const float* rp = raw + ((size_t)r * B + b) * BUDGET_Q * hw + (size_t)p;
        const BudgetMoments c = budget_moments(rp, hw, T);
        double v[10];
        v[7] = c.uu, v[8] = c.uv, v[9] = c.vv;
        if (inner) {
            const double kc = 0.5 * (c.uu + c.vv);
            double sxU = 0.0, syU = 0.0, sxV = 0.0, syV = 0.0, sxk = 0.0, syk = 0.0, sxt = 0.0, syt = 0.0, sxp = 0.0, syp = 0.0;
            double sxDu = 0.0, sxDv = 0.0, syDu = 0.0, syDv = 0.0, kl = 0.0, kr = 0.0, kd = 0.0, ku = 0.0;
#pragma unroll
            for (int i = -1; i <= 1; ++i) {
#pragma unroll
                for (int j = -1; j <= 1; ++j) {
                    if (i == 0 && j == 0) continue;
                    const long long o = (long long)i * Ww + j;
                    const BudgetMoments n = budget_moments(rp + o, hw, T);
                    const double* Mp = M + (size_t)b * 2 * hw + (size_t)(p + o);
                    const double U = Mp[0] + n.Du, Vv = Mp[hw] + n.Dv;
                    const double kk = 0.5 * (n.uu + n.vv);
                    const double wx = (double)(j * (i == 0 ? 2 : 1)), wy = (double)(i * (j == 0 ? 2 : 1));
                    if (j != 0) {
                        sxU = sxU + wx * U, sxV = sxV + wx * Vv, sxk = sxk + wx * kk, sxt = sxt + wx * (n.uuu + n.uvv);
                        sxp = sxp + wx * n.pu, sxDu = sxDu + wx * n.Du, sxDv = sxDv + wx * n.Dv;
                    }
                    if (i != 0) {
                        syU = syU + wy * U, syV = syV + wy * Vv, syk = syk + wy * kk, syt = syt + wy * (n.uuv + n.vvv);
                        syp = syp + wy * n.pv, syDu = syDu + wy * n.Du, syDv = syDv + wy * n.Dv;
                    }
                    if (i == 0 && j == -1) kl = kk;
                    if (i == 0 && j == 1) kr = kk;
                    if (i == -1 && j == 0) kd = kk;
                    if (i == 1 && j == 0) ku = kk;
                }
            }
            const double* Mc = M + (size_t)b * 2 * hw + (size_t)p;
            const double U = Mc[0] + c.Du, Vv = Mc[hw] + c.Dv;
            const double gx = ((double)rp[12 * hw] / T - sxDu * sxDu) - sxDv * sxDv;
            const double gy = ((double)rp[13 * hw] / T - syDu * syDu) - syDv * syDv;
            v[0] = -(U * (sxk / ex) + Vv * (syk / ey));
            v[1] = -((c.uu * (sxU / ex) + c.uv * (syU / ey + sxV / ex)) + c.vv * (syV / ey));
            v[2] = -0.5 * (sxt / ex + syt / ey);
            v[3] = -((sxp / ex + syp / ey) / fl.rho);
            v[4] = fl.nu * (((kr - 2.0 * kc) + kl) / dx2 + ((ku - 2.0 * kc) + kd) / dy2);
            v[5] = -(fl.nu * (gx / (64.0 * dx2) + gy / (64.0 * dy2)));
            v[6] = ((((v[0] + v[1]) + v[2]) + v[3]) + v[4]) + v[5];
        } else {
#pragma unroll
            for (int i = 0; i < 7; ++i) v[i] = nanv;
        }
        if (r < S) {
            const double rn = 1.0 / (double)(r + 1);
#pragma unroll
            for (int i = 0; i < 10; ++i) {
                const double d = v[i] - mean[i];
                mean[i] = mean[i] + d * rn;
                m2[i] = m2[i] + d * (v[i] - mean[i]);
            }
            if (mbud) {
#pragma unroll
                for (int i = 0; i < 7; ++i) mbud[(((size_t)b * S + r) * 7 + i) * hw + (size_t)p] = (float)v[i];
            }
        } else {
#pragma unroll
            for (int i = 0; i < 7; ++i) tbud[((size_t)b * 7 + i) * hw + (size_t)p] = (float)v[i];
#pragma unroll
            for (int i = 0; i < 3; ++i) tstr[((size_t)b * 3 + i) * hw + (size_t)p] = (float)v[7 + i];
        }
    }
    const double rs = 1.0 / (double)S;
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        bmean[((size_t)b * 7 + i) * hw + (size_t)p] = (float)mean[i];
        bstd[((size_t)b * 7 + i) * hw + (size_t)p] = (float)sqrt((m2[i] < 0.0 ? 0.0 : m2[i]) * rs);   // (a NaN m2 stays NaN: the frame)
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        smean[((size_t)b * 3 + i) * hw + (size_t)p] = (float)mean[7 + i];
        sstd[((size_t)b * 3 + i) * hw + (size_t)p] = (float)sqrt((m2[7 + i] < 0.0 ? 0.0 : m2[7 + i]) * rs);
    }
}

static int budget_sizes(int64_t S, int64_t B, int64_t Hh, int64_t Ww) {
    if (S < 1 || B < 1 || Hh < 3 || Ww < 3) return -1;
    if (S > BUDGET_MAXS || B > 65535 || Hh >= (1ll << 31) || Ww >= (1ll << 31) || Hh * Ww >= (1ll << 31) - 4 * BUDGET_THREADS ||
        (S + 1) * B * BUDGET_Q * Hh * Ww >= (1ll << 40))
        return -2;
    return 0;
}

extern "C" int tmg_ens_budget_plan(const int64_t* dims, int64_t* plan) {
    if (!dims) return -3;
    const int rc = budget_sizes(dims[0], dims[1], dims[2], dims[3]);
    if (rc != 0) return rc;
    if (!plan) return -3;
    const BudgetPlan g = budget_plan(dims[2], dims[3], 1);
    plan[0] = g.tile;
    plan[1] = g.tiles;
    plan[2] = g.vec;
    plan[3] = 0;
    return 0;
}

extern "C" int tmg_ens_budget_accum(const void* rows, const int64_t* t_d, const void* a, const void* m, void* raw, const int64_t* dims,
                                    hipStream_t st) {
    if (!dims) return -3;
    const int64_t k = dims[0], S = dims[1], B = dims[2], Hh = dims[3], Ww = dims[4], row0 = dims[5], t_before = dims[6];
    int rc = budget_sizes(S, B, Hh, Ww);
    if (rc == -1) return rc;
    if (k < 1 || row0 < 0 || row0 + k > S + 1 || t_before < 0) return -1;
    if (t_d && (t_d[1] < 0 || t_d[0] < t_d[1] + 3)) return -1;
    if (rc != 0) return rc;
    if (t_d && (t_d[0] >= (1ll << 31) || k * B * Hh * Ww * t_d[0] >= (1ll << 40))) return -2;
    if (!rows || !t_d || !a || !raw) return -3;
    const float* yr = (const float*)rows + t_d[1];
    const BudgetPlan g = budget_plan(Hh, Ww, ((uintptr_t)raw & 15) == 0);
    const dim3 grid((unsigned)g.tiles, (unsigned)B);
#define BUDGET_LAUNCH(V_)                                                                                                            \
    hipLaunchKernelGGL((ens_budget_accum_kernel<V_>), grid, dim3(BUDGET_THREADS), 0, st, yr, (int)t_d[0], (const float*)a,           \
                       (const float*)m, (float*)raw, (int)k, (int)B, (int)Hh, (int)Ww, (int)row0, (int)(t_before == 0))
    if (g.vec) BUDGET_LAUNCH(1);
    else BUDGET_LAUNCH(0);
#undef BUDGET_LAUNCH
    TMG_CHECK_LAUNCH();
    return 0;
}

extern "C" int tmg_ens_budget_terms(const void* raw, const void* M, const double* fl, void* budget_mean, void* budget_std,
                                    void* target_budget, void* stress_mean, void* stress_std, void* target_stress, void* member_budget,
                                    const int64_t* dims, hipStream_t st) {
    if (!dims) return -3;
    const int64_t S = dims[0], B = dims[1], Hh = dims[2], Ww = dims[3], T = dims[4];
    int rc = budget_sizes(S, B, Hh, Ww);
    if (rc == -1) return rc;
    if (T < 1) return -1;
    if (fl && (!(fl[0] > 0.0) || !(fl[1] > 0.0) || !(fl[2] >= 0.0) || !(fl[3] > 0.0) || !(fl[0] <= 1.0e300) || !(fl[1] <= 1.0e300) ||
               !(fl[2] <= 1.0e300) || !(fl[3] <= 1.0e300)))
        return -1;
    if (rc != 0) return rc;
    if (T >= (1ll << 31)) return -2;
    if (!raw || !M || !fl || !budget_mean || !budget_std || !target_budget || !stress_mean || !stress_std || !target_stress) return -3;
    const BudgetFl f = {fl[0], fl[1], fl[2], fl[3]};
    const dim3 grid((unsigned)((Hh * Ww + BUDGET_THREADS - 1) / BUDGET_THREADS), (unsigned)B);
    hipLaunchKernelGGL(ens_budget_terms_kernel, grid, dim3(BUDGET_THREADS), 0, st, (const float*)raw, (const double*)M, f,
                       (float*)budget_mean, (float*)budget_std, (float*)target_budget, (float*)stress_mean, (float*)stress_std,
                       (float*)target_stress, (float*)member_budget, (int)S, (int)B, (int)Hh, (int)Ww, (int)T);
    TMG_CHECK_LAUNCH();
    return 0;
}
