// Ensemble calibration scores of sampled roll-outs against the target (tmg_ops.EnsembleScores / utils.modelPredScores): per pixel the
// continuous ranked probability score of the S members x_1..x_S against the target y,
//   crps      = a ((1/S) sum_m |x_m - y| - (1 / (2 S^2))     sum_m sum_n |x_m - x_n|)
//   crps_fair = a ((1/S) sum_m |x_m - y| - (1 / (2 S (S-1))) sum_m sum_n |x_m - x_n|)        (S = 1: the pair term is 0)
// and the rank of the target among the members, rank = #{m : x_m < y} (strict), counted into a histogram of S + 1 bins per (case,
// step, channel).  x and y are the raw normalised fields; a = u[b][c] out_std[c] > 0 is the un-normalisation's scale (its offset
// out_mu cancels in every term, and a > 0 keeps the order, so the rank needs no arithmetic at all).
//   ens_score_store_kernel   one chunk of k members, NHWC -> rows m0 .. m0 + k - 1 of the planar member buffer xs [S][B][C][HW]
//   ens_score_step_kernel    once per kept step, after the step's last chunk is stored: scores, ranks, running time means
// One thread owns one pixel of one (case, channel); xs, the outputs and the time means are planar ([..][HW], lanes on consecutive
// pixels), so all their traffic is coalesced.  No float atomics: the only atomics are int32 adds of the rank histogram (LDS per
// block, then one global add per non-empty bin and block), whose sums do not depend on their order: bitwise reproducible.
//
// The pair sum P = sum_{m<n} |x_m - x_n| (every unordered pair once: sum_m sum_n = 2 P) holds SCORE_R members in registers and streams
// the later members past them: S + S^2 / (2 SCORE_R) loads per element instead of S^2 / 2.  Sum order, which the tests' rounding count
// is derived from (tests/test_scores_gpu.py):
//   per register block (members m0 .. m0 + SCORE_R - 1, m0 a multiple of SCORE_R):
//     a1      = sum over the block's members, in order, of |x_i - y|                                      (<= SCORE_R terms)
//     acc[i]  = one accumulator per held member i: |x_i - x_j| for the later members j of the block in order, then |x_i - x_n| for
//               the streamed members n = m0 + SCORE_R .. S - 1 in order                                   (<= S - 1 terms)
//     ap      = acc[0] + acc[1] + .. + acc[SCORE_R - 1]                                                   (SCORE_R - 1 additions)
//   over the blocks in order: t1 += a1, tp += ap                                                          (ceil(S / SCORE_R) each)
//   crps = a (t1 (1/S) - tp (1/S^2)), crps_fair = a (t1 (1/S) - tp (1/(S (S-1)))): rounded products (contraction off), the three
//   coefficients rounded once from fp64 on the host.
// Longest fp32 accumulation chain: (S - 1) + (SCORE_R - 1) + ceil(S / SCORE_R) additions for the pair term, min(SCORE_R, S) +
// ceil(S / SCORE_R) for the first term - not the S^2 / 2 of one accumulator.
// The running time means are plain fp32 running means in place, mean += (v - mean) / (t_before + 1): three roundings per step.
#include "tmg_common.h"
#include "tmglow_hip.h"

#define SCORE_MAXC 4
#define SCORE_R 8
#define SCORE_MAXS 1024      // the block's LDS histogram holds SCORE_MAXS + 1 int32 bins

__global__ __launch_bounds__(256) void ens_score_store_kernel(const float* __restrict__ y, int ps, float* __restrict__ xs, int B, int HW,
                                                              int C, int m0) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y, j = blockIdx.z;
    if (p >= HW) return;
    const size_t hw = (size_t)HW;
    const float* yp = y + ((size_t)(j * B + b) * hw + p) * ps;
    float* xp = xs + ((size_t)(m0 + j) * B + b) * C * hw + p;
#pragma unroll
    for (int c = 0; c < SCORE_MAXC; ++c)
        if (c < C) xp[(size_t)c * hw] = yp[c];
}

extern "C" int tmg_ens_score_store(const void* y, const int64_t* y_d, void* xs, const int64_t* dims, hipStream_t st) {
    const int64_t k = dims[0], B = dims[1], HW = dims[2], C = dims[3], S = dims[4], m0 = dims[5];
    if (k < 1 || B < 1 || HW < 1 || C < 2 || C > SCORE_MAXC || S < 1 || m0 < 0 || m0 + k > S) return -1;
    if (y_d[0] < C || y_d[1] < 0 || y_d[1] + C > y_d[0]) return -1;
    if (S > SCORE_MAXS || HW >= (1ll << 31) - 256 || B > 65535 || y_d[0] >= (1ll << 31)) return -2;
    if ((k * B) * HW * y_d[0] >= (1ll << 40) || S * B * C * HW >= (1ll << 40)) return -2;
    if (!y || !xs) return -3;
    dim3 grid((unsigned)((HW + 255) / 256), (unsigned)B, (unsigned)k);
    hipLaunchKernelGGL(ens_score_store_kernel, grid, dim3(256), 0, st, (const float*)y + y_d[1], (int)y_d[0], (float*)xs, (int)B, (int)HW,
                       (int)C, (int)m0);
    TMG_CHECK_LAUNCH();
    return 0;
}

__global__ __launch_bounds__(256) void ens_score_step_kernel(const float* __restrict__ xs, const float* __restrict__ tgt, int tps,
                                                             const float* __restrict__ scale, float* __restrict__ crps,
                                                             float* __restrict__ crps_fair, int* __restrict__ hist,
                                                             float* __restrict__ tcrps, float* __restrict__ tcrps_fair, long long ocs,
                                                             long long hcs, int S, int B, int HW, int C, int t_before, int flags,
                                                             float c1, float cp, float cpf) {
#pragma clang fp contract(off)
    __shared__ int bins[SCORE_MAXS + 1];
    const int p = blockIdx.x * 256 + threadIdx.x;
    const int c = blockIdx.y, b = blockIdx.z;
    for (int r = threadIdx.x; r <= S; r += 256) bins[r] = 0;
    __syncthreads();
    if (p < HW) {
        const size_t hw = (size_t)HW;
        const size_t ms = (size_t)B * C * hw;                                  // one member of xs
        const float* xp = xs + ((size_t)b * C + c) * hw + p;
        const float y = tgt[((size_t)b * hw + p) * tps + c];
        float t1 = 0.f, tp = 0.f;
        int below = 0;
        for (int m0 = 0; m0 < S; m0 += SCORE_R) {
            const int nr = min(SCORE_R, S - m0);
            float r[SCORE_R], acc[SCORE_R];
#pragma unroll
            for (int i = 0; i < SCORE_R; ++i) {
                r[i] = i < nr ? xp[(size_t)(m0 + i) * ms] : 0.f;
                acc[i] = 0.f;
            }
            float a1 = 0.f;
#pragma unroll
            for (int i = 0; i < SCORE_R; ++i) {
                if (i < nr) {
                    a1 += fabsf(r[i] - y);
                    below += r[i] < y ? 1 : 0;
                }
            }
#pragma unroll
            for (int i = 0; i < SCORE_R; ++i) {
#pragma unroll
                for (int j = i + 1; j < SCORE_R; ++j)
                    if (j < nr) acc[i] += fabsf(r[i] - r[j]);
            }
#pragma unroll 4
            for (int n = m0 + SCORE_R; n < S; ++n) {                           // only behind a full block: nr == SCORE_R
                const float v = xp[(size_t)n * ms];
#pragma unroll
                for (int i = 0; i < SCORE_R; ++i) acc[i] += fabsf(r[i] - v);
            }
            float ap = acc[0];
#pragma unroll
            for (int i = 1; i < SCORE_R; ++i) ap += acc[i];
            t1 += a1;
            tp += ap;
        }
        const float a = scale[b * C + c];
        const float first = t1 * c1;
        const float v0 = a * (first - tp * cp), v1 = a * (first - tp * cpf);
        const size_t o = (size_t)b * ocs + (size_t)c * hw + p;
        crps[o] = v0;
        crps_fair[o] = v1;
        if (flags & 1) {
            const size_t i = ((size_t)b * C + c) * hw + p;
            const float tn = 1.f / (float)(t_before + 1);
            float m0v = 0.f, m1v = 0.f;
            if (t_before > 0) {
                m0v = tcrps[i];
                m1v = tcrps_fair[i];
            }
            tcrps[i] = m0v + (v0 - m0v) * tn;
            tcrps_fair[i] = m1v + (v1 - m1v) * tn;
        }
        atomicAdd(&bins[below], 1);
    }
    __syncthreads();
    int* hp = hist + (size_t)b * hcs + (size_t)c * (S + 1);
    for (int r = threadIdx.x; r <= S; r += 256) {
        const int n = bins[r];
        if (n) atomicAdd(hp + r, n);
    }
}

extern "C" int tmg_ens_score_step(const void* xs, const void* target, const int64_t* t_d, const void* scale, void* crps, void* crps_fair,
                                  void* hist, void* tcrps, void* tcrps_fair, const int64_t* o_d, const int64_t* dims, hipStream_t st) {
    const int64_t S = dims[0], B = dims[1], HW = dims[2], C = dims[3], t_before = dims[4], flags = dims[5];
    if (S < 1 || B < 1 || HW < 1 || C < 2 || C > SCORE_MAXC || t_before < 0) return -1;
    if (t_d[0] < C || t_d[1] < 0 || t_d[1] + C > t_d[0]) return -1;
    if (o_d[0] < C * HW || o_d[1] < C * (S + 1)) return -1;
    if (S > SCORE_MAXS || HW >= (1ll << 31) - 256 || B > 65535 || t_d[0] >= (1ll << 31)) return -2;
    if (B * HW * t_d[0] >= (1ll << 40)|| S * B * C * HW >= (1ll << 40) || B * o_d[0] >= (1ll << 40) || B * o_d[1] >= (1ll << 40))
        return -2;
    if (!xs || !target || !scale || !crps || !crps_fair || !hist) return -3;
    if ((flags & 1) && (!tcrps || !tcrps_fair)) return -3;
    const double s = (double)S;
    dim3 grid((unsigned)((HW + 255) / 256), (unsigned)C, (unsigned)B);
    hipLaunchKernelGGL(ens_score_step_kernel, grid, dim3(256), 0, st, (const float*)xs, (const float*)target + t_d[1], (int)t_d[0],
                       (const float*)scale, (float*)crps, (float*)crps_fair, (int*)hist, (float*)tcrps, (float*)tcrps_fair,
                       (long long)o_d[0], (long long)o_d[1], (int)S, (int)B, (int)HW, (int)C, (int)t_before, (int)flags,
                       (float)(1.0 / s), (float)(1.0 / (s * s)), S > 1 ? (float)(1.0 / (s * (s - 1.0))) : 0.f);
    TMG_CHECK_LAUNCH();
    return 0;
}
