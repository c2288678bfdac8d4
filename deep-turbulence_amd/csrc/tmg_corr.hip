// Two-point space-time correlations of sampled roll-outs and of the target about probe points (tmg_ops.EnsembleCorrelation /
// utils.modelPredCorrelation):  R(x0; x, tau) = < u'_i(x0, t) u'_j(x, t + tau) >.  Rows are the S members plus the target as row S.
// With d_c = fl(a_c fl(y_c - m_c)), c = 0, 1, 2 (one subtraction, one multiplication), P probes, Q channel pairs (ci at the probe, cj
// in the field), L lags tau_l in timed steps and J the sorted set of distinct cj:
//   ens_corr_probe_kernel      one thread per (row of the chunk, case, probe, channel): series[row][b][t][p][c] = d_c at the probe.
//   ens_corr_accum_kernel<V>   one thread per pixel (V = 0) or per four consecutive pixels of one field row (V = 1) of a case; it loops
//                              over the chunk's k rows, forms d once per row and walks the LIVE planes of raw [S + 1][B][NPL][HW]
//                              (those of the lags with tau_l <= t) in groups of up to 16.  THE ORDER, stated once:
//                                X[p,q,l]: term = fl(series[row][b][t - tau_l][p][ci_q] * d_{cj_q})    F[j,l]: d_j    G[j,l]: fl(d_j d_j)
//                              and raw = fl(raw + term), one addition per timed step t >= tau_l in step order; at t == tau_l the term
//                              itself is stored, so the state needs no memset and a lag with tau_l >= T leaves its planes unwritten.
//                              Every operation is rounded on its own (no contraction): a float32 host mirror gives the same bits.
//                              The list of live planes (plane, kind, channel, store-or-add, the offset of the series value) is made
//                              by the launch body and handed over by value, so the lag gate and the store-or-add choice are uniform
//                              across the launch and every series value is a uniform scalar load.  All loads of a group are issued
//                              before the group's arithmetic and its stores come last.  An element of raw is touched by one thread
//                              once per call: no atomics, no LDS, no partial sums; the state is bitwise reproducible and does not
//                              depend on the chunking.  The kernel is bound by its state: at the defaults 40 planes read and written
//                              per row and step against 12 bytes of input.
//   ens_corr_finalize_kernel   once per mini-batch: one thread per (case, pixel), fp64; per (p, q, l) it loops over the S + 1 rows,
//                              forms cov and rho from X, F, G and the probe's fp64 tables pm, pv, carries a Welford mean / M2 over
//                              the members in member order and writes the lines through the probe for every row.
#include "tmg_common.h"
#include "tmglow_hip.h"
#include "tmglow_hip_corr.h"

#define CORR_MAXS 1024
#define CORR_THREADS 256
#define CORR_MAXP 8
#define CORR_MAXQ 4
#define CORR_MAXL 8
#define CORR_MAXLAG 64
#define CORR_MAXNPL (CORR_MAXP * CORR_MAXQ * CORR_MAXL + 2 * 3 * CORR_MAXL)
#define CORR_GROUP 16

struct CorrPlan {
    int64_t tile, tiles, vec, npl, offx, offf, offg;
};

// vec_ok: the base of raw is 16-byte aligned.  Four pixels per thread must lie in one field row: W % 4 == 0 (then H W % 4 == 0 and
// every plane starts 16-byte aligned).
static CorrPlan corr_plan(int64_t Hh, int64_t Ww, int64_t P, int64_t Q, int64_t L, int64_t J, int vec_ok) {
    CorrPlan g;
    const int64_t HW = Hh * Ww;
    g.vec = (vec_ok && Ww % 4 == 0) ? 1 : 0;
    g.tile = g.vec ? 4 * CORR_THREADS : CORR_THREADS;
    g.tiles = (HW + g.tile - 1) / g.tile;
    g.offx = 0;
    g.offf = P * Q * L;
    g.offg = g.offf + J * L;
    g.npl = g.offg + J * L;
    return g;
}

// The host's parsed cfg: what the three launches need of it.
struct CorrCfg {
    int P, Q, L, J;
    int ph[CORR_MAXP], pw[CORR_MAXP];
    int ci[CORR_MAXQ], cj[CORR_MAXQ], jx[CORR_MAXQ];                          // jx: the index of cj in J
    int tau[CORR_MAXL];
};

// One live plane of a call: lo = the offset of its series value inside the row's [steps][P][3] block; hi = plane | kind << 9 |
// channel << 11 | store << 13  (kind 0: X, 1: F, 2: G).
struct CorrLive {
    int n, pad;
    unsigned long long e[CORR_MAXNPL];
};

// What the finalize kernel needs per (p, q, l).
struct CorrFin {
    int P, Q, L, J;
    int ph[CORR_MAXP], pw[CORR_MAXP];
    int jx[CORR_MAXQ];
    int nl[CORR_MAXL];
};

__global__ __launch_bounds__(CORR_THREADS) void ens_corr_probe_kernel(const float* __restrict__ y, int ps, const float* __restrict__ a,
                                                                      const float* __restrict__ m, float* __restrict__ series, CorrFin cf,
                                                                      int k, int B, int HW, int Ww, int row0, int t, long long steps) {
#pragma clang fp contract(off)
    const int P = cf.P;
    const long long i = (long long)blockIdx.x * CORR_THREADS + threadIdx.x;
    if (i >= (long long)k * B * P * 3) return;
    const int c = (int)(i % 3);
    const int p = (int)((i / 3) % P);
    const int b = (int)((i / (3 * P)) % B);
    const int s = (int)(i / ((long long)3 * P * B));
    int pix = 0;
#pragma unroll
    for (int j = 0; j < CORR_MAXP; ++j)
        if (j == p) pix = cf.ph[j] * Ww + cf.pw[j];
    const float x = y[((size_t)((size_t)s * B + b) * HW + (size_t)pix) * ps + c];
    const float mv = m ? m[((size_t)b * 3 + c) * HW + (size_t)pix] : 0.f;
    const float tt = x - mv;
    series[((((size_t)(row0 + s) * B + b) * (size_t)steps + (size_t)t) * P + p) * 3 + c] = a[b * 3 + c] * tt;
}

template <int V>
__global__ __launch_bounds__(CORR_THREADS) void ens_corr_accum_kernel(const float* __restrict__ y, int ps, const float* __restrict__ a,
                                                                      const float* __restrict__ m, const float* __restrict__ series,
                                                                      float* __restrict__ raw, CorrLive lv, int k, int B, int HW, int row0,
                                                                      int NPL, long long sblock) {
#pragma clang fp contract(off)
    constexpr int PX = V ? 4 : 1;
    const long long p = ((long long)blockIdx.x * CORR_THREADS + threadIdx.x) * PX;
    const int b = blockIdx.y;
    if (p >= HW) return;                                                       // (V: W % 4 == 0, so p + 3 is in the same row)
    const size_t hw = (size_t)HW;
    const float a0 = a[b * 3], a1 = a[b * 3 + 1], a2 = a[b * 3 + 2];
    float m0[PX], m1[PX], m2[PX];
#pragma unroll
    for (int j = 0; j < PX; ++j) {
        m0[j] = m ? m[((size_t)b * 3) * hw + (size_t)p + j] : 0.f;
        m1[j] = m ? m[((size_t)b * 3 + 1) * hw + (size_t)p + j] : 0.f;
        m2[j] = m ? m[((size_t)b * 3 + 2) * hw + (size_t)p + j] : 0.f;
    }
    const int n = lv.n;
    for (int s = 0; s < k; ++s) {
        float* rp = raw + ((size_t)(row0 + s) * B + b) * (size_t)NPL * hw + (size_t)p;
        const float* sp = series + ((size_t)(row0 + s) * B + b) * (size_t)sblock;
        const float* yp = y + ((size_t)((size_t)s * B + b) * hw + (size_t)p) * ps;
        float d0[PX], d1[PX], d2[PX];
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            const float t0 = yp[(size_t)j * ps] - m0[j], t1 = yp[(size_t)j * ps + 1] - m1[j], t2 = yp[(size_t)j * ps + 2] - m2[j];
            d0[j] = a0 * t0, d1[j] = a1 * t1, d2[j] = a2 * t2;
        }
        for (int g0 = 0; g0 < n; g0 += CORR_GROUP) {
            float r[CORR_GROUP][PX], sv[CORR_GROUP];
#pragma unroll
            for (int i = 0; i < CORR_GROUP; ++i) {                             // all loads of the group first
                if (g0 + i < n) {
                    const unsigned long long e = lv.e[g0 + i];
                    const unsigned hi = (unsigned)(e >> 32);
                    const size_t pl = hi & 511u;
                    sv[i] = ((hi >> 9) & 3u) == 0u ? sp[(unsigned)e] : 0.f;
                    if (!((hi >> 13) & 1u)) {
                        if constexpr (V) {
                            const float4 q = *reinterpret_cast<const float4*>(rp + pl * hw);
                            r[i][0] = q.x, r[i][1] = q.y, r[i][2] = q.z, r[i][3] = q.w;
                        } else {
                            r[i][0] = rp[pl * hw];
                        }
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < CORR_GROUP; ++i) {
                if (g0 + i < n) {
                    const unsigned hi = (unsigned)(lv.e[g0 + i] >> 32);
                    const unsigned kind = (hi >> 9) & 3u, ch = (hi >> 11) & 3u;
                    const bool store = (hi >> 13) & 1u;
#pragma unroll
                    for (int j = 0; j < PX; ++j) {
                        const float dj = ch == 0u ? d0[j] : (ch == 1u ? d1[j] : d2[j]);
                        const float term = kind == 0u ? sv[i] * dj : (kind == 1u ? dj : dj * dj);
                        r[i][j] = store ? term : r[i][j] + term;
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < CORR_GROUP; ++i) {                             // the group's stores last
                if (g0 + i < n) {
                    const size_t pl = (unsigned)(lv.e[g0 + i] >> 32) & 511u;
                    if constexpr (V) *reinterpret_cast<float4*>(rp + pl * hw) = make_float4(r[i][0], r[i][1], r[i][2], r[i][3]);
                    else rp[pl * hw] = r[i][0];
                }
            }
        }
    }
}

__global__ __launch_bounds__(CORR_THREADS) void ens_corr_finalize_kernel(const float* __restrict__ raw, const double* __restrict__ pm,
                                                                         const double* __restrict__ pv, float* __restrict__ cmean,
                                                                         float* __restrict__ cstd, float* __restrict__ rmean,
                                                                         float* __restrict__ rstd, float* __restrict__ tcov,
                                                                         float* __restrict__ trho, float* __restrict__ mrho,
                                                                         float* __restrict__ linex, float* __restrict__ liney, CorrFin cf,
                                                                         int S, int B, int Hh, int Ww, int NPL) {
#pragma clang fp contract(off)
    const int HW = Hh * Ww;
    const long long p = (long long)blockIdx.x * CORR_THREADS + threadIdx.x;
    const int b = blockIdx.y;
    if (p >= HW) return;
    const int h = (int)(p / Ww), w = (int)(p - (long long)h * Ww);
    const size_t hw = (size_t)HW;
    const int P = cf.P, Q = cf.Q, L = cf.L, J = cf.J;
    const int offf = P * Q * L, offg = offf + J * L;
    const double nanv = __builtin_nan("");
    const double rs = 1.0 / (double)S;
    for (int pi = 0; pi < P; ++pi) {
        const bool onx = h == cf.ph[pi], ony = w == cf.pw[pi];
        for (int q = 0; q < Q; ++q) {
            const int j = cf.jx[q];
            for (int l = 0; l < L; ++l) {
                const int nl = cf.nl[l];
                const double n = (double)nl;
                const size_t idx = ((size_t)pi * Q + q) * L + l;
                double mc = 0.0, m2c = 0.0, mr = 0.0, m2r = 0.0;
                for (int r = 0; r <= S; ++r) {
                    double cov = nanv, rho = nanv;
                    if (nl >= 2) {                                             // (uniform) else no plane is read
                        const float* rp = raw + ((size_t)r * B + b) * (size_t)NPL * hw + (size_t)p;
                        const double X = (double)rp[idx * hw], F = (double)rp[(size_t)(offf + j * L + l) * hw];
                        const double G = (double)rp[(size_t)(offg + j * L + l) * hw];
                        const size_t ti = (((size_t)r * B + b) * P + pi) * Q * L + (size_t)q * L + l;
                        const double pmv = pm[ti], pvv = pv[ti];
                        const double mf = F / n;
                        const double vf = G / n - mf * mf;
                        cov = X / n - pmv * mf;
                        if (pvv > 0.0 && vf > 0.0) rho = cov / sqrt(pvv * vf);
                    }
                    const size_t li = ((size_t)b * (S + 1) + r) * P * Q * L + idx;
                    if (onx) linex[li * Ww + w] = (float)rho;
                    if (ony) liney[li * Hh + h] = (float)rho;
                    if (r < S) {
                        const double rn = 1.0 / (double)(r + 1);
                        const double dc = cov - mc;
                        mc = mc + dc * rn;
                        m2c = m2c + dc * (cov - mc);
                        const double dr = rho - mr;
                        mr = mr + dr * rn;
                        m2r = m2r + dr * (rho - mr);
                        if (mrho) mrho[(((size_t)b * S + r) * P * Q * L + idx) * hw + (size_t)p] = (float)rho;
                    } else {
                        const size_t o = ((size_t)b * P * Q * L + idx) * hw + (size_t)p;
                        tcov[o] = (float)cov;
                        trho[o] = (float)rho;
                    }
                }
                const size_t o = ((size_t)b * P * Q * L + idx) * hw + (size_t)p;
                cmean[o] = (float)mc;
                cstd[o] = (float)sqrt((m2c < 0.0 ? 0.0 : m2c) * rs);           // (a NaN m2 stays NaN)
                rmean[o] = (float)mr;
                rstd[o] = (float)sqrt((m2r < 0.0 ? 0.0 : m2r) * rs);
            }
        }
    }
}

static int corr_sizes(int64_t S, int64_t B, int64_t Hh, int64_t Ww, int64_t P, int64_t Q, int64_t L, int64_t J) {
    if (S < 1 || B < 1 || Hh < 1 || Ww < 1 || P < 1 || Q < 1 || L < 1 || J < 1 || J > 3 || J > Q) return -1;
    if (S > CORR_MAXS || B > 65535 || P > CORR_MAXP || Q > CORR_MAXQ || L > CORR_MAXL || Hh >= (1ll << 31) || Ww >= (1ll << 31) ||
        Hh * Ww >= (1ll << 31) - 4 * CORR_THREADS || (S + 1) * B * (P * Q * L + 2 * J * L) * Hh * Ww >= (1ll << 40))
        return -2;
    return 0;
}

// cfg -> c.  The counts are checked before anything behind them is read.
static int corr_parse(const int64_t* cfg, int64_t Hh, int64_t Ww, CorrCfg* c) {
    const int64_t P = cfg[0], Q = cfg[1], L = cfg[2];
    if (P < 1 || Q < 1 || L < 1) return -1;
    if (P > CORR_MAXP || Q > CORR_MAXQ || L > CORR_MAXL) return -2;
    c->P = (int)P, c->Q = (int)Q, c->L = (int)L;
    const int64_t* v = cfg + 3;
    for (int i = 0; i < P; ++i, v += 2) {
        if (v[0] < 0 || v[0] >= Hh || v[1] < 0 || v[1] >= Ww) return -1;
        c->ph[i] = (int)v[0], c->pw[i] = (int)v[1];
    }
    bool used[3] = {false, false, false};
    for (int i = 0; i < Q; ++i, v += 2) {
        if (v[0] < 0 || v[0] > 2 || v[1] < 0 || v[1] > 2) return -1;
        c->ci[i] = (int)v[0], c->cj[i] = (int)v[1];
        used[v[1]] = true;
    }
    int jof[3], J = 0;
    for (int ch = 0; ch < 3; ++ch) jof[ch] = used[ch] ? J++ : -1;
    c->J = J;
    for (int i = 0; i < Q; ++i) c->jx[i] = jof[c->cj[i]];
    for (int i = 0; i < L; ++i)
        if (i == 0 ? v[i] != 0 : v[i] <= v[i - 1]) return -1;
    if (v[L - 1] > CORR_MAXLAG) return -2;
    for (int i = 0; i < L; ++i) c->tau[i] = (int)v[i];
    return 0;
}

static CorrFin corr_fin(const CorrCfg& c, int64_t T) {
    CorrFin f = {};
    f.P = c.P, f.Q = c.Q, f.L = c.L, f.J = c.J;
    for (int i = 0; i < c.P; ++i) f.ph[i] = c.ph[i], f.pw[i] = c.pw[i];
    for (int i = 0; i < c.Q; ++i) f.jx[i] = c.jx[i];
    for (int i = 0; i < c.L; ++i) f.nl[i] = (int)(T - c.tau[i] < 0 ? 0 : T - c.tau[i]);
    return f;
}

extern "C" int tmg_ens_corr_plan(const int64_t* dims, int64_t* plan) {
    if (!dims) return -3;
    const int rc = corr_sizes(dims[0], dims[1], dims[2], dims[3], dims[4], dims[5], dims[6], dims[7]);
    if (rc != 0) return rc;
    if (!plan) return -3;
    const CorrPlan g = corr_plan(dims[2], dims[3], dims[4], dims[5], dims[6], dims[7], 1);
    plan[0] = g.tile;
    plan[1] = g.tiles;
    plan[2] = g.vec;
    plan[3] = g.npl;
    plan[4] = g.offx;
    plan[5] = g.offf;
    plan[6] = g.offg;
    plan[7] = 0;
    return 0;
}

// The checks the probe and the accumulate launch share: dims = {k, S, B, H, W, row0, t, steps}.
static int corr_feed_checks(const int64_t* t_d, const int64_t* cfg, const int64_t* dims, CorrCfg* c) {
    const int64_t k = dims[0], S = dims[1], B = dims[2], Hh = dims[3], Ww = dims[4], row0 = dims[5], t = dims[6], steps = dims[7];
    if (S < 1 || B < 1 || Hh < 1 || Ww < 1) return -1;
    int rc = corr_parse(cfg, Hh, Ww, c);
    if (rc == -1) return rc;
    if (k < 1 || row0 < 0 || row0 + k > S + 1 || t < 0 || steps < 1 || t >= steps) return -1;
    if (t_d && (t_d[1] < 0 || t_d[0] < t_d[1] + 3)) return -1;
    if (rc != 0) return rc;
    rc = corr_sizes(S, B, Hh, Ww, c->P, c->Q, c->L, c->J);
    if (rc != 0) return rc;
    if (steps * c->P * 3 >= (1ll << 31) || (S + 1) * B * steps * c->P * 3 >= (1ll << 40)) return -2;
    if (t_d && (t_d[0] >= (1ll << 31) || k * B * Hh * Ww * t_d[0] >= (1ll << 40))) return -2;
    return 0;
}

extern "C" int tmg_ens_corr_probe(const void* rows, const int64_t* t_d, const void* a, const void* m, void* series, const int64_t* cfg,
                                  const int64_t* dims, hipStream_t st) {
    if (!dims || !cfg) return -3;
    CorrCfg c = {};
    const int rc = corr_feed_checks(t_d, cfg, dims, &c);
    if (rc != 0) return rc;
    if (!rows || !t_d || !a || !series) return -3;
    const int64_t k = dims[0], B = dims[2], Hh = dims[3], Ww = dims[4], row0 = dims[5], t = dims[6], steps = dims[7];
    const CorrFin f = corr_fin(c, 0);
    const int64_t total = k * B * c.P * 3;
    const dim3 grid((unsigned)((total + CORR_THREADS - 1) / CORR_THREADS));
    hipLaunchKernelGGL(ens_corr_probe_kernel, grid, dim3(CORR_THREADS), 0, st, (const float*)rows + t_d[1], (int)t_d[0], (const float*)a,
                       (const float*)m, (float*)series, f, (int)k, (int)B, (int)(Hh * Ww), (int)Ww, (int)row0, (int)t, (long long)steps);
    TMG_CHECK_LAUNCH();
    return 0;
}

extern "C" int tmg_ens_corr_accum(const void* rows, const int64_t* t_d, const void* a, const void* m, const void* series, void* raw,
                                  const int64_t* cfg, const int64_t* dims, hipStream_t st) {
    if (!dims || !cfg) return -3;
    CorrCfg c = {};
    const int rc = corr_feed_checks(t_d, cfg, dims, &c);
    if (rc != 0) return rc;
    if (!rows || !t_d || !a || !series || !raw) return -3;
    const int64_t k = dims[0], B = dims[2], Hh = dims[3], Ww = dims[4], row0 = dims[5], t = dims[6], steps = dims[7];
    const CorrPlan g = corr_plan(Hh, Ww, c.P, c.Q, c.L, c.J, ((uintptr_t)raw & 15) == 0);
    // the live planes of this call: the lags with tau_l <= t; a plane is stored at t == tau_l
    CorrLive lv;
    lv.n = 0, lv.pad = 0;
    auto put = [&](int64_t plane, unsigned kind, unsigned ch, int l, unsigned soff) {
        const unsigned hi = (unsigned)plane | kind << 9 | ch << 11 | (t == c.tau[l] ? 1u : 0u) << 13;
        lv.e[lv.n++] = (unsigned long long)hi << 32 | soff;
    };
    int jch[3], J = 0;
    for (int ch = 0; ch < 3; ++ch)
        for (int q = 0; q < c.Q; ++q)
            if (c.cj[q] == ch) {
                jch[J++] = ch;
                break;
            }
    for (int p = 0; p < c.P; ++p)
        for (int q = 0; q < c.Q; ++q)
            for (int l = 0; l < c.L; ++l)
                if (c.tau[l] <= t)
                    put(g.offx + ((int64_t)p * c.Q + q) * c.L + l, 0u, (unsigned)c.cj[q], l,
                        (unsigned)(((t - c.tau[l]) * c.P + p) * 3 + c.ci[q]));
    for (int kind = 1; kind <= 2; ++kind)
        for (int j = 0; j < J; ++j)
            for (int l = 0; l < c.L; ++l)
                if (c.tau[l] <= t) put((kind == 1 ? g.offf : g.offg) + (int64_t)j * c.L + l, (unsigned)kind, (unsigned)jch[j], l, 0u);
    const float* yr = (const float*)rows + t_d[1];
    const dim3 grid((unsigned)g.tiles, (unsigned)B);
#define CORR_LAUNCH(V_)                                                                                                              \
    hipLaunchKernelGGL((ens_corr_accum_kernel<V_>), grid, dim3(CORR_THREADS), 0, st, yr, (int)t_d[0], (const float*)a, (const float*)m, \
                       (const float*)series, (float*)raw, lv, (int)k, (int)B, (int)(Hh * Ww), (int)row0, (int)g.npl,                 \
                       (long long)(steps * c.P * 3))
    if (g.vec) CORR_LAUNCH(1);
    else CORR_LAUNCH(0);
#undef CORR_LAUNCH
    TMG_CHECK_LAUNCH();
    return 0;
}

extern "C" int tmg_ens_corr_finalize(const void* raw, const void* pm, const void* pv, void* cov_mean, void* cov_std, void* rho_mean,
                                     void* rho_std, void* target_cov, void* target_rho, void* member_rho, void* line_x, void* line_y,
                                     const int64_t* cfg, const int64_t* dims, hipStream_t st) {
    if (!dims || !cfg) return -3;
    const int64_t S = dims[0], B = dims[1], Hh = dims[2], Ww = dims[3], T = dims[4];
    if (S < 1 || B < 1 || Hh < 1 || Ww < 1) return -1;
    CorrCfg c = {};
    int rc = corr_parse(cfg, Hh, Ww, &c);
    if (rc == -1) return rc;
    if (T < 1) return -1;
    if (rc != 0) return rc;
    rc = corr_sizes(S, B, Hh, Ww, c.P, c.Q, c.L, c.J);
    if (rc != 0) return rc;
    if (T >= (1ll << 31)) return -2;
    if (!raw || !pm || !pv || !cov_mean || !cov_std || !rho_mean || !rho_std || !target_cov || !target_rho || !line_x || !line_y) return -3;
    const CorrPlan g = corr_plan(Hh, Ww, c.P, c.Q, c.L, c.J, 1);
    const CorrFin f = corr_fin(c, T);
    const dim3 grid((unsigned)((Hh * Ww + CORR_THREADS - 1) / CORR_THREADS), (unsigned)B);
    hipLaunchKernelGGL(ens_corr_finalize_kernel, grid, dim3(CORR_THREADS), 0, st, (const float*)raw, (const double*)pm, (const double*)pv,
                       (float*)cov_mean, (float*)cov_std, (float*)rho_mean, (float*)rho_std, (float*)target_cov, (float*)target_rho,
                       (float*)member_rho, (float*)line_x, (float*)line_y, f, (int)S, (int)B, (int)Hh, (int)Ww, (int)g.npl);
    TMG_CHECK_LAUNCH();
    return 0;
}
