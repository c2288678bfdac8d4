// Structure functions and variogram score of sampled roll-outs (tmg_ops.EnsembleStructure / utils.modelPredStructure): the dependence
// between neighbouring pixels of ONE member, which no per-pixel score sees and the energy score barely notices.  Per case b, kept step
// and channel c the rows are the S raw normalised members x_0..x_{S-1} (the planar buffer xs [S][B][C][HW] that tmg_ens_score_store
// fills) and the normalised target x_S := y (read from its NHWC channel slice).  A lag is l = (dx, dy) in pixels, dx along W and dy
// along H, in canonical form (dx >= 0, and dy > 0 when dx == 0); its pairs are all pixels p = (i, j) for which p' = (i + dy, j + dx)
// lies in the field, N_l = (H - |dy|) (W - dx) of them; D_m(p) = x_m(p') - x_m(p).
//   M_q[m] = sum_p D_m(p)^q, q = 2, 3, 4                                             the raw moment sums, per row m = 0..S and lag
//   s_m(p) = sqrtf(|D_m(p)|),  sbar(p) = (s_0 + .. + s_{S-1}, sequentially in member order) * fl(1 / S)
//   V_l = sum_p (s_S(p) - sbar(p))^2                                                 the raw variogram sum of order 1/2, per lag
//   ens_sfun_mom_kernel<LN>   one block per (pixel slice, row, case-channel): its partial M_2, M_3, M_4 of every lag into the workspace
//   ens_sfun_var_kernel<LN>   one block per (pixel slice, case-channel): its partial V of every lag into the workspace
//   ens_sfun_fold_kernel      the P slices' partials added in slice order into mom / vsum, and those added into tmom / tvar on a timed
//                             step (written, not read, at the first one)
// LN = 4, 8 or 16: the lags an instance holds accumulators for (L <= LN).
//
// Sum order, which the tests' rounding count is derived from (tests/structure_cases.py).  The H W pixels, numbered i W + j, are cut
// into P slices of SL pixels (SL a multiple of 256, the host's choice: tmg_ens_sfun_plan).  A pair belongs to the slice of its pixel
// p, wherever p' lies.  Thread t of the block's 256 takes the pixels t, t + 256, .. of the slice in order and adds the terms of its
// valid pairs to one accumulator per lag and moment (SL / 256 terms at most); the 64 accumulators of a wave are added as a butterfly
// (lane ^ 1, ^ 2, .. ^ 32: six additions deep, the same bits in every lane), the four waves in wave order (3 additions), the slices in
// slice order (P - 1 additions).  The plan reports Lc = SL / 256 + 9, the additions along the longest path inside one partial.  A term
// is D = fl(x' - x), D2 = fl(D D), then D2, fl(D2 D), fl(D2 D2); no product is contracted into a sum.  No float atomics anywhere: the
// same inputs give the same bits, for every chunking of the members.  Neighbour reads go to global memory: a member plane at the
// workload's shape is 128 KB and stays in L2, and rows are read coalesced along W.
#include "tmg_common.h"
#include "tmglow_hip.h"

#define SFUN_MAXC 4
#define SFUN_MAXS 1024
#define SFUN_MAXL 16                     // lags of one call
#define SFUN_MAXLAG 64                   // |dx|, |dy| of a lag
#define SFUN_SLQ 256                     // slice granularity: one pixel per thread
#define SFUN_MINSL 512                   // no more slices than HW / 512: two pixels per thread before the block reduces
#define SFUN_TARGET_BLOCKS 768           // the variogram grid the slice count aims at
#define SFUN_WS_CAP (1ll << 24)          // floats of workspace beyond which the slice count is cut (P = 1 may exceed it)
#define SFUN_PLAN_HEAD 8
#define SFUN_PLAN_LAG 5

// per lag: the flat offset dy W + dx of p', and the pixels whose pair is valid: j < jmax, ilo <= i < ihi
struct SfunLags {
    int off[SFUN_MAXL], jmax[SFUN_MAXL], ilo[SFUN_MAXL], ihi[SFUN_MAXL];
};

struct SfunPlan {
    int64_t P, Lc, ws, SL;
    int64_t N[SFUN_MAXL];
    SfunLags lg;
};

// lags [L][2] = (dx, dy): canonical, inside the field and the lag range, distinct; else false
static bool sfun_lags(const int64_t* lags, int64_t L, int64_t H, int64_t W, SfunPlan& g) {
    for (int l = 0; l < SFUN_MAXL; ++l) {
        g.N[l] = 0;
        g.lg.off[l] = 0;
        g.lg.jmax[l] = 0;
        g.lg.ilo[l] = 0;
        g.lg.ihi[l] = 0;
    }
    for (int64_t l = 0; l < L; ++l) {
        const int64_t dx = lags[2 * l], dy = lags[2 * l + 1], ady = dy < 0 ? -dy : dy;
        if (dx < 0 || dx > SFUN_MAXLAG || ady > SFUN_MAXLAG || (dx == 0 && dy <= 0) || dx >= W || ady >= H) return false;
        for (int64_t k = 0; k < l; ++k)
            if (lags[2 * k] == dx && lags[2 * k + 1] == dy) return false;
        g.lg.off[l] = (int)(dy * W + dx);
        g.lg.jmax[l] = (int)(W - dx);
        g.lg.ilo[l] = (int)(dy < 0 ? -dy : 0);
        g.lg.ihi[l] = (int)(dy > 0 ? H - dy : H);
        g.N[l] = (H - ady) * (W - dx);
    }
    return true;
}

static void sfun_slices(int64_t S, int64_t B, int64_t C, int64_t HW, int64_t L, SfunPlan& g) {
    const int64_t bc = B * C, per = bc * L * (3 * (S + 1) + 1);              // workspace floats of one slice
    const int64_t maxp = (HW + SFUN_MINSL - 1) / SFUN_MINSL;
    int64_t P = (SFUN_TARGET_BLOCKS + bc - 1) / bc;
    const int64_t pcap = SFUN_WS_CAP / per;
    if (P > pcap) P = pcap;
    if (P > maxp) P = maxp;
    if (P < 1) P = 1;
    const TmgSlices s = tmg_slices(HW, P, SFUN_SLQ);
    g.SL = s.SL;
    g.P = s.P;
    g.Lc = g.SL / SFUN_SLQ + 9;
    g.ws = per * g.P;
}

// (not tmg_common.h's wave_sum: this one adds in ASCENDING xor order, 1 up to 32, which gives other bits for floats)
__device__ __forceinline__ float sfun_wave_sum(float v) {
#pragma clang fp contract(off)
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);
    return v;
}

// the block's NQ LN accumulators, [moment][lag] with one per thread: wave butterflies, then the waves in wave order; lag l < L of
// moment q goes to dst[q L + l]
template <int NQ, int LN>
__device__ __forceinline__ void sfun_block_sum(float (&acc)[NQ * LN], float* __restrict__ dst, int L) {
#pragma clang fp contract(off)
    __shared__ float red[4][NQ * LN];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < NQ * LN; ++k) {
        if (k % LN < L) {                                                  // (uniform)
            const float v = sfun_wave_sum(acc[k]);
            if (lane == 0) red[wave][k] = v;
        }
    }
    __syncthreads();
    const int k = threadIdx.x, q = k / LN, l = k - q * LN;
    if (k < NQ * LN && l < L) dst[q * L + l] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
}

// ws moments part: [B C][R][P][3][L]
template <int LN>
__global__ __launch_bounds__(256) void ens_sfun_mom_kernel(const float* __restrict__ xs, const float* __restrict__ tgt, int tps,
                                                           float* __restrict__ ws, int S, int B, int C, int W, int HW, int SL, int P,
                                                           int L, SfunLags lg) {
#pragma clang fp contract(off)
    const int slice = blockIdx.x, m = blockIdx.y, bc = blockIdx.z;
    const int b = bc / C, c = bc - b * C;
    const size_t hw = (size_t)HW;
    const float* row = m < S ? xs + ((size_t)m * B * C + bc) * hw : tgt + (size_t)b * hw * tps + c;
    const size_t ps = m < S ? 1 : (size_t)tps;
    float acc[3 * LN];                                                     // [moment][lag]
#pragma unroll
    for (int k = 0; k < 3 * LN; ++k) acc[k] = 0.f;
    const int pbeg = slice * SL, pend = min(HW, pbeg + SL);
    for (int p = pbeg + (int)threadIdx.x; p < pend; p += 256) {
        const int i = p / W, j = p - i * W;
        const float x0 = row[(size_t)p * ps];
#pragma unroll
        for (int l = 0; l < LN; ++l) {
            if (l < L && j < lg.jmax[l] && i >= lg.ilo[l] && i < lg.ihi[l]) {
                const float d = row[(size_t)(p + lg.off[l]) * ps] - x0;
                const float d2 = d * d;
                acc[l] += d2;
                acc[LN + l] += d2 * d;
                acc[2 * LN + l] += d2 * d2;
            }
        }
    }
    sfun_block_sum<3, LN>(acc, ws + (((size_t)bc * (S + 1) + m) * P + slice) * (3 * L), L);
}

// ws variogram part: [B C][P][L]
template <int LN>
__global__ __launch_bounds__(256) void ens_sfun_var_kernel(const float* __restrict__ xs, const float* __restrict__ tgt, int tps,
                                                           float* __restrict__ wsv, int S, int B, int C, int W, int HW, int SL, int P,
                                                           int L, float inv_s, SfunLags lg) {
#pragma clang fp contract(off)
    const int slice = blockIdx.x, bc = blockIdx.y;
    const int b = bc / C, c = bc - b * C;
    const size_t hw = (size_t)HW, ms = (size_t)B * C * hw;
    const float* tbc = tgt + (size_t)b * hw * tps + c;
    float v[LN];
#pragma unroll
    for (int l = 0; l < LN; ++l) v[l] = 0.f;
    const int pbeg = slice * SL, pend = min(HW, pbeg + SL);
    for (int p = pbeg + (int)threadIdx.x; p < pend; p += 256) {
        const int i = p / W, j = p - i * W;
        bool ok[LN];
        float sum[LN];
#pragma unroll
        for (int l = 0; l < LN; ++l) {
            ok[l] = l < L && j < lg.jmax[l] && i >= lg.ilo[l] && i < lg.ihi[l];
            sum[l] = 0.f;
        }
        const float* xp = xs + (size_t)bc * hw + p;
        for (int m = 0; m < S; ++m, xp += ms) {
            const float x0 = xp[0];
#pragma unroll
            for (int l = 0; l < LN; ++l)
                if (ok[l]) sum[l] += sqrtf(fabsf(xp[lg.off[l]] - x0));     // (0 + s_0 is s_0)
        }
        const float t0 = tbc[(size_t)p * tps];
#pragma unroll
        for (int l = 0; l < LN; ++l) {
            if (ok[l]) {
                const float ss = sqrtf(fabsf(tbc[(size_t)(p + lg.off[l]) * tps] - t0));
                const float sbar = sum[l] * inv_s;
                const float e = ss - sbar;
                v[l] += e * e;
            }
        }
    }
    sfun_block_sum<1, LN>(v, wsv + ((size_t)bc * P + slice) * L, L);
}

// element e < 3 B C L R: mom [3][B][C][L][R]; then B C L elements of vsum [B][C][L]
__global__ __launch_bounds__(256) void ens_sfun_fold_kernel(const float* __restrict__ ws, float* __restrict__ mom, float* __restrict__ vsum,
                                                            float* __restrict__ tmom, float* __restrict__ tvar, int BC, int L, int R,
                                                            int P, int timed, int t_before) {
#pragma clang fp contract(off)
    const size_t nm = (size_t)3 * BC * L * R, nv = (size_t)BC * L;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= nm + nv) return;
    const float* src;
    size_t stride;
    float *out, *tout;
    if (e < nm) {
        const int m = (int)(e % R);
        size_t k = e / R;
        const int l = (int)(k % L);
        k /= L;
        const int bc = (int)(k % BC), q = (int)(k / BC);
        stride = (size_t)3 * L;
        src = ws + ((size_t)bc * R + m) * P * stride + (size_t)q * L + l;
        out = mom + e;
        tout = tmom + e;
    } else {
        const size_t k = e - nm;
        stride = (size_t)L;
        src = ws + (size_t)BC * R * P * 3 * L + (k / L) * P * stride + k % L;
        out = vsum + k;
        tout = tvar + k;
    }
    float a = src[0];
    for (int s = 1; s < P; ++s) a += src[(size_t)s * stride];
    *out = a;
    if (timed) *tout = t_before > 0 ? *tout + a : a;
}

static int sfun_check(int64_t S, int64_t B, int64_t C, int64_t H, int64_t W, int64_t L) {
    if (S < 1 || B < 1 || H < 1 || W < 1 || C < 2 || C > SFUN_MAXC || L < 1 || L > SFUN_MAXL) return -1;
    return 0;
}

static int sfun_ranges(int64_t S, int64_t B, int64_t C, int64_t H, int64_t W) {
    if (S > SFUN_MAXS || H >= (1ll << 31) || W >= (1ll << 31) || H * W >= (1ll << 31) - 256 || B * C > 65535 ||
        S * B * C * H * W >= (1ll << 40))
        return -2;
    return 0;
}

extern "C" int tmg_ens_sfun_plan(const int64_t* dims, const int64_t* lags, int64_t* plan) {
    const int64_t S = dims[0], B = dims[1], C = dims[2], H = dims[3], W = dims[4], L = dims[5];
    SfunPlan g;
    if (sfun_check(S, B, C, H, W, L) != 0) return -1;
    if (lags && !sfun_lags(lags, L, H, W, g)) return -1;
    if (sfun_ranges(S, B, C, H, W) != 0) return -2;
    if (!lags || !plan) return -3;
    sfun_slices(S, B, C, H * W, L, g);
    if (g.ws >= (1ll << 40)) return -2;
    plan[0] = g.P;
    plan[1] = g.Lc;
    plan[2] = g.ws;
    plan[3] = g.SL;
    plan[4] = 256;
    plan[5] = L;
    plan[6] = S + 1;
    plan[7] = 0;
    for (int l = 0; l < SFUN_MAXL; ++l) {
        int64_t* q = plan + SFUN_PLAN_HEAD + SFUN_PLAN_LAG * l;
        q[0] = g.lg.off[l];
        q[1] = g.lg.jmax[l];
        q[2] = g.lg.ilo[l];
        q[3] = g.lg.ihi[l];
        q[4] = g.N[l];
    }
    return 0;
}

extern "C" int tmg_ens_sfun_step(const void* xs, const void* target, const int64_t* t_d, const int64_t* lags, void* ws, int64_t ws_floats,
                                 void* mom, void* vsum, void* tmom, void* tvar, const int64_t* dims, hipStream_t st) {
    const int64_t S = dims[0], B = dims[1], C = dims[2], H = dims[3], W = dims[4], L = dims[5], t_before = dims[6], flags = dims[7];
    const bool timed = flags & 1;
    SfunPlan g;
    if (sfun_check(S, B, C, H, W, L) != 0 || t_before < 0) return -1;
    if (lags && !sfun_lags(lags, L, H, W, g)) return -1;
    if (t_d && (t_d[0] < C || t_d[1] < 0 || t_d[1] + C > t_d[0])) return -1;
    if (sfun_ranges(S, B, C, H, W) != 0) return -2;
    const int64_t HW = H * W;
    if (t_d && (t_d[0] >= (1ll << 31) || B * HW * t_d[0] >= (1ll << 40))) return -2;
    if (!lags || !t_d) return -3;
    sfun_slices(S, B, C, HW, L, g);
    if (g.ws >= (1ll << 40)) return -2;
    if (ws_floats < g.ws) return -1;
    if (!xs || !target || !ws || !mom || !vsum) return -3;
    if (timed && (!tmom || !tvar)) return -3;
    const float* tg = (const float*)target + t_d[1];
    const int R = (int)S + 1, BC = (int)(B * C);
    float* wsv = (float*)ws + (size_t)BC * R * g.P * 3 * L;
    const dim3 gm((unsigned)g.P, (unsigned)R, (unsigned)BC), gv((unsigned)g.P, (unsigned)BC);
#define SFUN_LAUNCH(LN_)                                                                                                              \
    do {                                                                                                                              \
        hipLaunchKernelGGL(ens_sfun_mom_kernel<LN_>, gm, dim3(256), 0, st, (const float*)xs, tg, (int)t_d[0], (float*)ws, (int)S,     \
                           (int)B, (int)C, (int)W, (int)HW, (int)g.SL, (int)g.P, (int)L, g.lg);                                        \
        TMG_CHECK_LAUNCH();                                                                                                           \
        hipLaunchKernelGGL(ens_sfun_var_kernel<LN_>, gv, dim3(256), 0, st, (const float*)xs, tg, (int)t_d[0], wsv, (int)S, (int)B,    \
                           (int)C, (int)W, (int)HW, (int)g.SL, (int)g.P, (int)L, (float)(1.0 / (double)S), g.lg);                      \
        TMG_CHECK_LAUNCH();                                                                                                           \
    } while (0)
    if (L <= 4) SFUN_LAUNCH(4);
    else if (L <= 8) SFUN_LAUNCH(8);
    else SFUN_LAUNCH(16);
#undef SFUN_LAUNCH
    const int64_t n = (3 * (int64_t)R + 1) * BC * L;
    hipLaunchKernelGGL(ens_sfun_fold_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const float*)ws, (float*)mom,
                       (float*)vsum, (float*)tmom, (float*)tvar, BC, (int)L, R, (int)g.P, timed ? 1 : 0, (int)t_before);
    TMG_CHECK_LAUNCH();
    return 0;
}
