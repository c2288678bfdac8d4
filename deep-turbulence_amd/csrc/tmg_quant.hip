// Prediction intervals of sampled roll-outs (tmg_ops.EnsembleQuantiles / utils.modelPredQuantiles): per pixel the exact order
// statistics of the S members x_0..x_{S-1} at up to QUANT_MAXQ probability levels (numpy's method="linear"), exceedance probabilities
// against up to QUANT_MAXK thresholds, and their aggregates over the timed steps.  The members are the raw normalised fields in the
// planar buffer xs [S][B][C][HW] that tmg_ens_score_store (tmg_scores.hip) fills; sc * out_std > 0 keeps the order, so selection on
// the raw values is selection on the physical ones and only the selected values are un-normalised.
//   ens_quant_step_kernel    once per kept step, after the step's last chunk is stored
// One thread owns one pixel of one (case, channel), as ens_score_step_kernel; xs and every output are planar ([..][HW], lanes on
// consecutive pixels): all traffic is coalesced.  No LDS and no atomics: every thread owns its outputs and counters, so the result is
// bitwise reproducible.
//
// Selection by rank counting.  rank_m = #{n : x_n < x_m} + #{n < m : x_n == x_m} is a permutation of 0..S-1 (ties go by member index).
// QUANT_R members are held in registers and all S members stream past them: a streamed member n before the block adds (v <= r_i), one
// behind the block adds (v < r_i), inside the block the index decides which of the two.  S^2 / QUANT_R loads and two vector
// instructions (compare, add-with-carry) per pair.  The <= 2 QUANT_MAXQ wanted ranks (lo_j, hi_j of every level, slots 2 j and
// 2 j + 1) come with the kernel arguments, so they are wave-uniform; a held member whose rank equals a wanted one is copied into that
// slot.  The slots start as NaN: a rank that no member takes (possible only with non-finite members) shows.
// All register arrays (r, rank, slot, count) are indexed by compile-time constants in fully unrolled loops: no scratch.
//   qraw_j = x_(lo) + w_j (x_(hi) - x_(lo))           subtraction, product, addition: three rounded operations (contraction off)
//   quant  = sc * fmaf(out_std, qraw_j, out_mu)       tmg_unnorm_fma (tmg_field.h)
//   exceed = float(count) * float(1 / S)              one rounded product; every member is counted once, while it is held
//   tquant: fp32 running mean in place, m += (quant - m) * (1 / (t_before + 1)); tbelow += (y < qraw_j); texceed += count
#include "tmg_field.h"
#include "tmglow_hip.h"

#define QUANT_MAXC 4
#define QUANT_R 8
#define QUANT_MAXQ 8
#define QUANT_NW (2 * QUANT_MAXQ)
#define QUANT_MAXK 4
#define QUANT_MAXS 1024

struct QuantArgs {
    int want[QUANT_NW];      // slot 2 j: lo_j, slot 2 j + 1: hi_j
    float w[QUANT_MAXQ];
    int ech[QUANT_MAXK];     // the thresholds' channels
    int egt[QUANT_MAXK];     // 1: count x > thr, 0: count x < thr
};

__global__ __launch_bounds__(256) void ens_quant_step_kernel(const float* __restrict__ xs, const float* __restrict__ tgt, int tps,
                                                             const float* __restrict__ u, const float* __restrict__ out_mu,
                                                             const float* __restrict__ out_std, const float* __restrict__ thr,
                                                             float* __restrict__ quant, float* __restrict__ exceed,
                                                             float* __restrict__ tquant, int* __restrict__ tbelow,
                                                             int* __restrict__ texceed, long long ocs, long long ecs, int S, int B, int HW,
                                                             int C, int Q, int K, int t_before, int flags, float inv_s, QuantArgs a) {
#pragma clang fp contract(off)
    const int p = blockIdx.x * 256 + threadIdx.x;
    const int c = blockIdx.y, b = blockIdx.z;
    if (p >= HW) return;
    const size_t hw = (size_t)HW;
    const size_t ms = (size_t)B * C * hw;                                      // one member of xs
    const float* xp = xs + ((size_t)b * C + c) * hw + p;
    const int NW = 2 * Q;
    float slot[QUANT_NW];
#pragma unroll
    for (int j = 0; j < QUANT_NW; ++j) slot[j] = __builtin_nanf("");
    float th[QUANT_MAXK];
    int cnt[QUANT_MAXK];
    bool mine[QUANT_MAXK];
#pragma unroll
    for (int k = 0; k < QUANT_MAXK; ++k) {
        mine[k] = k < K && a.ech[k] == c;                                      // block-uniform
        th[k] = mine[k] ? thr[(size_t)b * K + k] : 0.f;
        cnt[k] = 0;
    }
    for (int m0 = 0; m0 < S; m0 += QUANT_R) {
        const int nr = min(QUANT_R, S - m0);
        float r[QUANT_R];
        int rank[QUANT_R];
#pragma unroll
        for (int i = 0; i < QUANT_R; ++i) {
            r[i] = i < nr ? xp[(size_t)(m0 + i) * ms] : 0.f;
            rank[i] = 0;
        }
#pragma unroll
        for (int k = 0; k < QUANT_MAXK; ++k) {
            if (mine[k]) {
#pragma unroll
                for (int i = 0; i < QUANT_R; ++i)
                    if (i < nr) cnt[k] += (a.egt[k] ? r[i] > th[k] : r[i] < th[k]) ? 1 : 0;
            }
        }
#pragma unroll
        for (int i = 0; i < QUANT_R; ++i) {                                    // inside the block the index decides
#pragma unroll
            for (int j = 0; j < QUANT_R; ++j) {
                if (j < i) rank[i] += (j < nr && r[j] <= r[i]) ? 1 : 0;
                if (j > i) rank[i] += (j < nr && r[j] < r[i]) ? 1 : 0;
            }
        }
#pragma unroll 4
        for (int n = 0; n < m0; ++n) {                                         // the members before the block: ties count
            const float v = xp[(size_t)n * ms];
#pragma unroll
            for (int i = 0; i < QUANT_R; ++i) rank[i] += v <= r[i] ? 1 : 0;
        }
#pragma unroll 4
        for (int n = m0 + QUANT_R; n < S; ++n) {                               // the members behind it (nr == QUANT_R): ties do not
            const float v = xp[(size_t)n * ms];
#pragma unroll
            for (int i = 0; i < QUANT_R; ++i) rank[i] += v < r[i] ? 1 : 0;
        }
#pragma unroll
        for (int i = 0; i < QUANT_R; ++i) {
#pragma unroll
            for (int j = 0; j < QUANT_NW; ++j)
                if (i < nr && j < NW && rank[i] == a.want[j]) slot[j] = r[i];
        }
    }
    const float sc = u ? u[b * C + c] : 1.f;
    const float sd = out_std[c], mu = out_mu[c];
    const bool timed = flags & 1, scored = flags & 2;
    const float y = scored ? tgt[((size_t)b * hw + p) * tps + c] : 0.f;
    const float tn = 1.f / (float)(t_before + 1);
    float* qp = quant + (size_t)b * ocs + (size_t)c * hw + p;
    const size_t ti = ((size_t)b * Q * C + c) * hw + p;
#pragma unroll
    for (int j = 0; j < QUANT_MAXQ; ++j) {
        if (j < Q) {
            const float lo = slot[2 * j], hi = slot[2 * j + 1];
            const float d = hi - lo;
            const float wd = a.w[j] * d;
            const float qraw = lo + wd;
            const float v = tmg_unnorm_fma(qraw, sc, sd, mu);
            const size_t lv = (size_t)j * C * hw;
            qp[lv] = v;
            if (timed) {
                const float m = t_before > 0 ? tquant[ti + lv] : 0.f;
                tquant[ti + lv] = m + (v - m) * tn;
                if (scored) tbelow[ti + lv] = (t_before > 0 ? tbelow[ti + lv] : 0) + (y < qraw ? 1 : 0);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < QUANT_MAXK; ++k) {
        if (mine[k]) {
            exceed[(size_t)b * ecs + (size_t)k * hw + p] = (float)cnt[k] * inv_s;
            if (timed) {
                const size_t ei = ((size_t)b * K + k) * hw + p;
                texceed[ei] = (t_before > 0 ? texceed[ei] : 0) + cnt[k];
            }
        }
    }
}

extern "C" int tmg_ens_quant_step(const void* xs, const void* target, const int64_t* t_d, const void* u, const void* out_mu,
                                  const void* out_std, const int64_t* lohi, const float* w, const void* thr, const int64_t* ex, void* quant,
                                  void* exceed, void* tquant, void* tbelow, void* texceed, const int64_t* o_d, const int64_t* dims,
                                  hipStream_t st) {
    const int64_t S = dims[0], B = dims[1], HW = dims[2], C = dims[3], Q = dims[4], K = dims[5], t_before = dims[6], flags = dims[7];
    const bool timed = flags & 1, scored = flags & 2;
    if (S < 1 || B < 1 || HW < 1 || C < 2 || C > QUANT_MAXC || Q < 1 || Q > QUANT_MAXQ || K < 0 || K > QUANT_MAXK || t_before < 0) return -1;
    if (lohi)
        for (int64_t j = 0; j < 2 * Q; ++j)
            if (lohi[j] < 0 || lohi[j] > S - 1) return -1;
    if (ex)
        for (int64_t k = 0; k < K; ++k)
            if (ex[2 * k] < 0 || ex[2 * k] > C - 1 || ex[2 * k + 1] < 0 || ex[2 * k + 1] > 1) return -1;
    if (scored && t_d && (t_d[0] < C || t_d[1] < 0 || t_d[1] + C > t_d[0])) return -1;
    if (o_d[0] < Q * C * HW || o_d[1] < K * HW) return -1;
    if (S > QUANT_MAXS || HW >= (1ll << 31) - 256 || B > 65535) return -2;
    if (scored && t_d && (t_d[0] >= (1ll << 31) || B * HW * t_d[0] >= (1ll << 40))) return -2;
    if (S * B * C * HW >= (1ll << 40) || B * o_d[0] >= (1ll << 40) || B * o_d[1] >= (1ll << 40)) return -2;
    if (!xs || !out_mu || !out_std || !lohi || !w || !quant) return -3;
    if (scored && (!target || !t_d)) return -3;
    if (K > 0 && (!thr || !ex || !exceed)) return -3;
    if (timed && (!tquant || (scored && !tbelow) || (K > 0 && !texceed))) return -3;
    QuantArgs a;
    for (int j = 0; j < QUANT_NW; ++j) a.want[j] = j < 2 * Q ? (int)lohi[j] : -1;
    for (int j = 0; j < QUANT_MAXQ; ++j) a.w[j] = j < Q ? w[j] : 0.f;
    for (int k = 0; k < QUANT_MAXK; ++k) {
        a.ech[k] = k < K ? (int)ex[2 * k] : -1;
        a.egt[k] = k < K ? (int)ex[2 * k + 1] : 0;
    }
    dim3 grid((unsigned)((HW + 255) / 256), (unsigned)C, (unsigned)B);
    hipLaunchKernelGGL(ens_quant_step_kernel, grid, dim3(256), 0, st, (const float*)xs, scored ? (const float*)target + t_d[1] : nullptr,
                       scored ? (int)t_d[0] : 0, (const float*)u, (const float*)out_mu, (const float*)out_std, (const float*)thr,
                       (float*)quant, (float*)exceed, (float*)tquant, (int*)tbelow, (int*)texceed, (long long)o_d[0], (long long)o_d[1],
                       (int)S, (int)B, (int)HW, (int)C, (int)Q, (int)K, (int)t_before, (int)flags, (float)(1.0 / (double)S), a);
    TMG_CHECK_LAUNCH();
    return 0;
}
