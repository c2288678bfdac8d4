// Multivariate rank histograms of sampled roll-outs (tmg_ops.EnsembleFieldRanks / utils.modelPredFieldRanks): the pre-ranks of the
// average-rank and band-depth histograms of Thorarinsdottir, Scheuerer & Heinz (2016), the depth being the modified band depth of
// Lopez-Pintado & Romo (2009).  The rows are the S members x_0..x_{S-1} and the target x_S, raw normalised fp32 in the planar buffer
// xs [S + 1][B][C][HW] that tmg_ens_score_store (tmg_scores.hip) fills; ranks do not change under u * out_std > 0 and out_mu, so there
// is no arithmetic on the values at all, only comparisons.  Per pixel and row i, over the S OTHER rows j != i:
//   lt = #{j : x_j < x_i}, eq = #{j : x_j == x_i}, gt = S - lt - eq
//   A  = 2 lt + eq                                twice the mid-rank minus a constant
//   D  = C(S,2) - C(lt,2) - C(gt,2)               the pairs of other rows whose closed band [min, max] holds x_i
//   O  = [lt == S or gt == S], target row only    the target lies strictly outside the members' range
//   ens_frank_step_kernel   once per kept step, after the step's last chunk and the target are stored: per block of 256 pixels of
//                           one (case, channel) the sums of A and D of every row and of O, into the block's record of the workspace
//                           ws [B][C][nblk][2 (S + 1) + 1] int32; O also goes into the int32 plane tout [B][C][HW] of the timed steps
//   ens_frank_fold_kernel   the records of one (case, channel) summed over the blocks in block order, as int64, into
//                           pre_raw [B][Tk][C][S + 1][2] and outside [B][Tk][C] at step t
// One thread owns one pixel of one (case, channel); xs and tout are planar ([..][HW], lanes on consecutive pixels): all their traffic
// is coalesced.  No atomics: every word of ws, pre_raw, outside and tout has one writer, and every sum is an integer sum, so the
// result is bitwise reproducible and equal to an int64 reference.
//
// Rank counting as in tmg_quant.hip: FRANK_R rows are held in registers and all S + 1 rows stream past them, two counters (<, ==)
// per held row; a held row skips itself by its compile-time index, every row outside the held block is another row.
// (S + 1)^2 / FRANK_R loads per pixel.  All register arrays (r, lt, eq, val) are indexed by compile-time constants in fully unrolled
// loops: no scratch.
#include "tmg_common.h"
#include "tmglow_hip_frank.h"

#define FRANK_MAXC 4
#define FRANK_R 8
#define FRANK_NV (2 * FRANK_R + 1)     // the block's reduced values: A and D of the held rows, then O
#define FRANK_MAXS 1024

#define FRANK_G 4                      // streamed rows loaded together; divides FRANK_R

// One streamed row against the held rows: two counters per held row.
__device__ __forceinline__ void frank_count(float v, const float (&r)[FRANK_R], int (&lt)[FRANK_R], int (&eq)[FRANK_R]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < FRANK_R; ++i) {
        lt[i] += v < r[i] ? 1 : 0;
        eq[i] += v == r[i] ? 1 : 0;
    }
}

__global__ __launch_bounds__(256) void ens_frank_step_kernel(const float* __restrict__ xs, int* __restrict__ ws, int* __restrict__ tout,
                                                             int S, int B, int HW, int C, int nblk, int t_before, int timed) {
#pragma clang fp contract(off)
    __shared__ int red[4][FRANK_NV];
    const int p = blockIdx.x * 256 + threadIdx.x;
    const int c = blockIdx.y, b = blockIdx.z;
    // A lane past the field does NOT return: the kernel has barriers.  It loads the field's last pixel, contributes zeros and takes
    // part in every reduction and barrier.
    const bool valid = p < HW;
    const int pl = valid ? p : HW - 1;
    const size_t hw = (size_t)HW;
    const size_t ms = (size_t)B * C * hw;                                      // one row of xs
    const float* xp = xs + ((size_t)b * C + c) * hw + pl;
    const int Rn = S + 1;
    const int NV = 2 * Rn + 1;                                                 // the words of one record
    int* rec = ws + (((size_t)b * C + c) * nblk + blockIdx.x) * (size_t)NV;
    const int cs2 = S * (S - 1) / 2;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int m0 = 0; m0 < Rn; m0 += FRANK_R) {
        const int nr = min(FRANK_R, Rn - m0);
        float r[FRANK_R];
        int lt[FRANK_R], eq[FRANK_R];
#pragma unroll
        for (int i = 0; i < FRANK_R; ++i) {
            r[i] = i < nr ? xp[(size_t)(m0 + i) * ms] : 0.f;
            lt[i] = 0;
            eq[i] = 0;
        }
#pragma unroll
        for (int i = 0; i < FRANK_R; ++i) {                                    // inside the block: every held row but itself
#pragma unroll
            for (int j = 0; j < FRANK_R; ++j) {
                if (j != i) {
                    lt[i] += (j < nr && r[j] < r[i]) ? 1 : 0;
                    eq[i] += (j < nr && r[j] == r[i]) ? 1 : 0;
                }
            }
        }
        // The streamed rows come in groups of FRANK_G loads issued together, then counted: one wait per group, not per row.
        for (int n = 0; n < m0; n += FRANK_G) {                                // the rows before the block (m0 % FRANK_G == 0)
            float v[FRANK_G];
#pragma unroll
            for (int u = 0; u < FRANK_G; ++u) v[u] = xp[(size_t)(n + u) * ms];
#pragma unroll
            for (int u = 0; u < FRANK_G; ++u) frank_count(v[u], r, lt, eq);
        }
        int n = m0 + FRANK_R;                                                  // the rows behind it (nr == FRANK_R)
        for (; n + FRANK_G <= Rn; n += FRANK_G) {
            float v[FRANK_G];
#pragma unroll
            for (int u = 0; u < FRANK_G; ++u) v[u] = xp[(size_t)(n + u) * ms];
#pragma unroll
            for (int u = 0; u < FRANK_G; ++u) frank_count(v[u], r, lt, eq);
        }
        for (; n < Rn; ++n) frank_count(xp[(size_t)n * ms], r, lt, eq);
        // int32 is enough: per pixel A <= 2 S <= 2048 and D <= C(S,2) <= 523 776 (S <= 1024), so the sum over the block's 256
        // pixels is at most 256 * 523 776 = 134 086 656 < 2^31.
        int val[FRANK_NV];
        val[2 * FRANK_R] = 0;
        const bool has_target = m0 + nr == Rn;                                 // block-uniform: the target is the last row
#pragma unroll
        for (int i = 0; i < FRANK_R; ++i) {
            const int gt = S - lt[i] - eq[i];
            const bool on = valid && i < nr;
            val[2 * i] = on ? 2 * lt[i] + eq[i] : 0;
            val[2 * i + 1] = on ? cs2 - lt[i] * (lt[i] - 1) / 2 - gt * (gt - 1) / 2 : 0;
            if (has_target && i == nr - 1) {
                const int o = (valid && (lt[i] == S || gt == S)) ? 1 : 0;
                val[2 * FRANK_R] = o;
                if (timed && valid) {                                          // t_before == 0 stores: the plane needs no memset
                    const size_t ti = ((size_t)b * C + c) * hw + p;
                    tout[ti] = (t_before > 0 ? tout[ti] : 0) + o;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < FRANK_NV; ++k) val[k] = wave_sum(val[k]);
        __syncthreads();                                                       // the previous held block's sums are read
#pragma unroll
        for (int k = 0; k < FRANK_NV; ++k)
            if (lane == k) red[wv][k] = val[k];                                // every lane holds the wave's sum
        __syncthreads();
        if (threadIdx.x < FRANK_NV) {
            const int k = threadIdx.x;
            const int sum = red[0][k] + red[1][k] + red[2][k] + red[3][k];
            if (k < 2 * nr) rec[2 * m0 + k] = sum;
            if (k == 2 * FRANK_R && has_target) rec[2 * Rn] = sum;
        }
    }
}

__global__ __launch_bounds__(256) void ens_frank_fold_kernel(const int* __restrict__ ws, long long* __restrict__ pre_raw,
                                                             long long* __restrict__ outside, int NV, int nblk, int C, int Tk, int t) {
    const int c = blockIdx.x, b = blockIdx.y;
    const int* rp = ws + ((size_t)b * C + c) * nblk * (size_t)NV;
    const size_t o = ((size_t)b * Tk + t) * C + c;
    for (int k = threadIdx.x; k < NV; k += 256) {
        long long acc = 0;
        for (int q = 0; q < nblk; ++q) acc += (long long)rp[(size_t)q * NV + k];     // block order; lanes on consecutive words
        if (k < NV - 1) pre_raw[o * (size_t)(NV - 1) + k] = acc;
        else outside[o] = acc;
    }
}

struct FrankPlan { int64_t nblk, rec, ws; };

static int frank_plan(int64_t S, int64_t B, int64_t C, int64_t HW, FrankPlan& pl) {
    if (S < 1 || B < 1 || HW < 1 || C < 2 || C > FRANK_MAXC) return -1;
    if (S > FRANK_MAXS || HW >= (1ll << 31) - 256 || B > 65535 || (S + 1) * B * C * HW >= (1ll << 40)) return -2;
    pl.nblk = (HW + 255) / 256;
    pl.rec = 2 * (S + 1) + 1;
    pl.ws = B * C * pl.nblk * pl.rec;
    return 0;
}

extern "C" int tmg_ens_frank_plan(const int64_t* dims, int64_t* out) {
    if (!dims || !out) return -3;
    FrankPlan pl;
    const int rc = frank_plan(dims[0], dims[1], dims[2], dims[3], pl);
    if (rc) return rc;
    out[0] = pl.nblk;
    out[1] = pl.nblk;
    out[2] = dims[2];
    out[3] = dims[1];
    out[4] = 256;
    out[5] = pl.rec;
    out[6] = pl.ws;
    return 0;
}

extern "C" int tmg_ens_frank_step(const void* xs, void* ws, int64_t ws_words, void* pre_raw, void* outside, void* tout,
                                  const int64_t* dims, hipStream_t st) {
    if (!dims) return -3;
    const int64_t S = dims[0], B = dims[1], HW = dims[2], C = dims[3], Tk = dims[4], t = dims[5], t_before = dims[6], flags = dims[7];
    const bool timed = flags & 1;
    FrankPlan pl;
    const int rc = frank_plan(S, B, C, HW, pl);
    if (rc == -1 || Tk < 1 || t < 0 || t >= Tk || t_before < 0 || t_before >= (1ll << 31)) return -1;
    if (rc) return rc;
    if (B * Tk * C * (pl.rec - 1) >= (1ll << 40)) return -2;
    if (!xs || !ws || !pre_raw || !outside || (timed && !tout)) return -3;
    if (ws_words < pl.ws) return -1;
    dim3 grid((unsigned)pl.nblk, (unsigned)C, (unsigned)B);
    hipLaunchKernelGGL(ens_frank_step_kernel, grid, dim3(256), 0, st, (const float*)xs, (int*)ws, (int*)tout, (int)S, (int)B, (int)HW,
                       (int)C, (int)pl.nblk, (int)t_before, timed ? 1 : 0);
    TMG_CHECK_LAUNCH();
    hipLaunchKernelGGL(ens_frank_fold_kernel, dim3((unsigned)C, (unsigned)B), dim3(256), 0, st, (const int*)ws, (long long*)pre_raw,
                       (long long*)outside, (int)pl.rec, (int)pl.nblk, (int)C, (int)Tk, (int)t);
    TMG_CHECK_LAUNCH();
    return 0;
}
