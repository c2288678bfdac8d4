// Projection of sampled roll-outs on the target's POD modes (tmg_ops.EnsembleModes / utils.modelPredModes): do the members hold the
// reference's coherent structures, with the right energy and the right dynamics?  Per case b the host hands over three opaque fp32
// tables built once per mini-batch from the target series (tmg_ops.pod_basis): the scales a [B][Cg], the mean planes m [B][Cg][HW]
// and the K <= 16 modes psi [B][K][Cg][HW].  Per kept step and chunk, for every row (a member of the chunk, or the step's target):
//   d = fl(a_c fl(x - m))                          two fp32 roundings, no contraction
//   coef_raw[j] = sum_c sum_p d psi_j,  j < K       on the fp32 matrix pipe
//   en_raw      = sum_c sum_p d d                   beside it on the vector ALUs, from the same d
// A row's sums need no other row: the kernel reads the chunk's NHWC rows where sampleEnsemble left them and keeps no member buffer.
//   ens_pod_kernel<NTL>   one block per (pixel slice, group of 64 members, case): its partial sums, no atomics
//   ens_pod_fold_kernel   P > 1: the P slices' partials added in slice order (fp32); P = 1: the block writes the outputs itself
//
// Layout.  v_mfma_f32_16x16x4_f32 with the lane maps of tmg_symgram.h: A[i = l & 15][k = l >> 4], B[k = l >> 4][j = l & 15], D column
// l & 15, rows 4 (l >> 4) + 0..3.  The members are the M rows in tiles of 16, the modes the one N tile, pixels x channels the reduction.
// A wave takes 64 consecutive pixels of one channel at a time; lane (row, kq) holds the 16 CONSECUTIVE pixels kq 16 .. kq 16 + 15 of
// them and MFMA step s = 0..15 contracts element s of every lane's run (the order of the sum is free as long as A and B agree).
//   B (psi, planar): lane (mode, kq) loads its run as four float4 (HW a multiple of 4), as tmg_gram.hip loads its rows; the fragment
//     is built once per chunk and channel and serves the block's up to 4 member tiles.
//   A (the rows, NHWC with a member stride of B whole fields): a fragment-order load would have every lane walk a row of its own with
//     the pixel stride, 64 cache lines per instruction.  Instead lane l of the wave loads pixel l of the chunk for the 16 members of
//     the tile, one after the other (consecutive lanes on consecutive pixels, as every NHWC reader here; m is loaded once per pixel
//     and serves the 16 members), forms d and writes it to the wave's own LDS tile [16 members][64 pixels, row pitch 68]: a
//     conflict-free ds_write_b32.  The fragment is read back as four ds_read_b128 per lane; with the pitch of 68 floats the 16 lanes
//     of one kq land on 16 different 16-byte slots of the bank row.  Two tiles per wave alternate, so that one barrier per (tile,
//     channel) orders the write before the read and the read before the next write to the same tile; the loop counts are uniform
//     over the block (rows, pixels and modes that do not exist are zeros in LDS, never skipped), which keeps the barriers legal.
//
// Sum order, which the tests' rounding count is derived from (tests/modes_cases.py).  The pixels are cut into P slices of SL pixels
// (tmg_ens_pod_plan: a function of HW alone, so a row's result does not depend on the chunk it comes in).  Inside a slice wave w takes
// the chunks w, w + 4, ..; per chunk the channels in list order; an MFMA is a k-ordered fmaf chain onto its C input, so a coefficient's
// accumulator is a chain of SL Cg / 4 fmaf; the energy's is a chain of SL Cg / 16 fmaf per lane (kq), the four kq added in order.
// Waves 1..3 hand over through LDS and wave 0 adds in wave order, then the slices are added in slice order.  L = SL Cg terms per
// partial, L P >= HW Cg.  No float atomics anywhere.
#include "tmg_common.h"
#include "tmglow_hip.h"

#define POD_MAXK 16
#define POD_MAXC 4
#define POD_MAXS 1024
#define POD_MT 64                        // members of a block: 4 tiles of 16
#define POD_CHUNK 64                     // pixels a wave contracts per step
#define POD_SLQ 256                      // slice granularity: 4 waves x one chunk
#define POD_MAXP 32                      // slices at most
#define POD_PITCH 68                     // floats between two members' rows of an LDS tile
#define POD_ROW 17                       // floats of one row's partial: 16 modes, then the energy

struct PodChannels {
    int ch[POD_MAXC];
};

struct PodPlan {
    int64_t P, SL, L, ws;
};

static PodPlan pod_plan(int64_t S, int64_t B, int64_t Cg, int64_t HW) {
    PodPlan g;
    int64_t P = (HW + POD_SLQ - 1) / POD_SLQ;
    if (P > POD_MAXP) P = POD_MAXP;
    const TmgSlices s = tmg_slices(HW, P, POD_SLQ);
    g.SL = s.SL;
    g.P = s.P;
    g.L = g.SL * Cg;
    g.ws = g.P > 1 ? g.P * S * B * POD_ROW : 0;
    return g;
}

template <int NTL>
__global__ __launch_bounds__(256) void ens_pod_kernel(const float* __restrict__ y, int ps, PodChannels pc, const float* __restrict__ a,
                                                      const float* __restrict__ m, const float* __restrict__ psi, float* __restrict__ ws,
                                                      float* __restrict__ coef, float* __restrict__ en, long long cs_c, long long ms_c,
                                                      long long cs_e, long long ms_e, int k, int B, int HW, int Cg, int K, int SL, int P,
                                                      int vec) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) float stage[4][2][16 * POD_PITCH];                            // per wave two tiles [member][pixel]
    __shared__ float red[3][NTL * 5][64];                                      // waves 1..3: [accumulator register | energy][lane]
    const int wave = threadIdx.x >> 6, l = threadIdx.x & 63, l16 = l & 15, kq = l >> 4;
    const int slice = blockIdx.x, s0 = blockIdx.y * POD_MT, b = blockIdx.z;
    const int nt = min(NTL, (k - s0 + 15) >> 4);                               // the block's tiles that hold a member (>= 1)
    const size_t hw = (size_t)HW, ms = (size_t)B * hw * ps;                    // floats between two members of one case
    const float* yb = y + (size_t)b * hw * ps;                                 // member 0 of case b
    f32x4 acc[NTL];
    float e[NTL];
#pragma unroll
    for (int it = 0; it < NTL; ++it) {
        acc[it] = f32x4{0.f, 0.f, 0.f, 0.f};
        e[it] = 0.f;
    }
    const int pbeg = slice * SL, pend = min(HW, pbeg + SL);
    int q = 0;
    for (int pc0 = pbeg; pc0 < pend; pc0 += 4 * POD_CHUNK) {                   // the same count in every wave
        const int pcw = pc0 + wave * POD_CHUNK;
        const int pl = pcw + l;                                                // the pixel this lane loads
        const int p0 = pcw + kq * 16;                                          // the run this lane contracts
        for (int c = 0; c < Cg; ++c) {
            const int chn = c == 0 ? pc.ch[0] : c == 1 ? pc.ch[1] : c == 2 ? pc.ch[2] : pc.ch[3];   // (no indexed argument: no scratch)
            const float ac = a[b * Cg + c];
            const float mv = pl < HW ? m[((size_t)b * Cg + c) * hw + pl] : 0.f;
            float fb[16];
#pragma unroll
            for (int s = 0; s < 16; ++s) fb[s] = 0.f;
            if (l16 < K && p0 < HW) {
                const float* pr = psi + (((size_t)b * K + l16) * Cg + c) * hw + p0;
                if (vec && p0 + 16 <= HW) {
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const float4 t = *reinterpret_cast<const float4*>(pr + 4 * v);
                        fb[4 * v] = t.x;
                        fb[4 * v + 1] = t.y;
                        fb[4 * v + 2] = t.z;
                        fb[4 * v + 3] = t.w;
                    }
                } else {
#pragma unroll
                    for (int s = 0; s < 16; ++s)
                        if (p0 + s < HW) fb[s] = pr[s];
                }
            }
#pragma unroll
            for (int it = 0; it < NTL; ++it) {
                if (it < nt) {                                                 // uniform over the block
                    float* buf = stage[wave][q];
                    const float* yp = yb + (size_t)pl * ps + chn;
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int s = s0 + 16 * it + i;
                        float d = 0.f;
                        if (s < k && pl < HW) {
                            const float t = yp[(size_t)s * ms] - mv;
                            d = ac * t;
                        }
                        buf[i * POD_PITCH + l] = d;
                    }
                    __syncthreads();
                    float fa[16];
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const float4 t = *reinterpret_cast<const float4*>(buf + l16 * POD_PITCH + kq * 16 + 4 * v);
                        fa[4 * v] = t.x;
                        fa[4 * v + 1] = t.y;
                        fa[4 * v + 2] = t.z;
                        fa[4 * v + 3] = t.w;
                    }
#pragma unroll
                    for (int s = 0; s < 16; ++s) {
                        acc[it] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[s], fb[s], acc[it], 0, 0, 0);
                        e[it] = __builtin_fmaf(fa[s], fa[s], e[it]);
                    }
                    q ^= 1;
                }
            }
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int it = 0; it < NTL; ++it) {
#pragma unroll
            for (int v = 0; v < 4; ++v) red[wave - 1][it * 5 + v][l] = acc[it][v];
            red[wave - 1][it * 5 + 4][l] = e[it];
        }
    }
    __syncthreads();
    if (wave == 0) {
        const size_t rows = (size_t)k * B;
#pragma unroll
        for (int it = 0; it < NTL; ++it) {
            float ev = ((e[it] + red[0][it * 5 + 4][l]) + red[1][it * 5 + 4][l]) + red[2][it * 5 + 4][l];
            // the four pixel groups of a member in group order: lane l16 of every group holds the same member
            const float e0 = __shfl(ev, l16, 64), e1 = __shfl(ev, l16 + 16, 64), e2 = __shfl(ev, l16 + 32, 64), e3 = __shfl(ev, l16 + 48, 64);
            ev = ((e0 + e1) + e2) + e3;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const float t = ((acc[it][v] + red[0][it * 5 + v][l]) + red[1][it * 5 + v][l]) + red[2][it * 5 + v][l];
                const int s = s0 + 16 * it + 4 * kq + v;                       // D row 4 kq + v: the member; column l16: the mode
                if (it < nt && s < k && l16 < K) {
                    if (P > 1) ws[((size_t)slice * rows + (size_t)s * B + b) * POD_ROW + l16] = t;
                    else coef[(size_t)b * cs_c + (size_t)s * ms_c + l16] = t;
                }
            }
            const int s = s0 + 16 * it + l16;
            if (it < nt && kq == 0 && s < k) {
                if (P > 1) ws[((size_t)slice * rows + (size_t)s * B + b) * POD_ROW + 16] = ev;
                else en[(size_t)b * cs_e + (size_t)s * ms_e] = ev;
            }
        }
    }
}

// out = ws[0] + ws[1] + .. in slice order; thread (row, j): j < K a mode sum, j == K the energy
__global__ __launch_bounds__(256) void ens_pod_fold_kernel(const float* __restrict__ ws, float* __restrict__ coef, float* __restrict__ en,
                                                           long long cs_c, long long ms_c, long long cs_e, long long ms_e, int k, int B,
                                                           int K, int P) {
#pragma clang fp contract(off)
    const size_t rows = (size_t)k * B;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * (K + 1)) return;
    const size_t row = i / (K + 1);
    const int j = (int)(i - row * (K + 1));
    const int s = (int)(row / B), b = (int)(row - (size_t)s * B);
    const float* wp = ws + row * POD_ROW + (j < K ? j : 16);
    float t = wp[0];
    for (int sl = 1; sl < P; ++sl) t += wp[(size_t)sl * rows * POD_ROW];
    if (j < K) coef[(size_t)b * cs_c + (size_t)s * ms_c + j] = t;
    else en[(size_t)b * cs_e + (size_t)s * ms_e] = t;
}

static int pod_sizes(int64_t S, int64_t B, int64_t HW, int64_t Cg, int64_t K) {
    if (S < 1 || B < 1 || HW < 1 || Cg < 1 || Cg > POD_MAXC || K < 1 || K > POD_MAXK) return -1;
    if (S > POD_MAXS || B > 65535 || HW >= (1ll << 31) - 256 || S * B * HW >= (1ll << 40) || B * K * Cg * HW >= (1ll << 40)) return -2;
    return 0;
}

extern "C" int tmg_ens_pod_plan(const int64_t* dims, int64_t* plan) {
    if (!dims) return -3;
    const int64_t S = dims[0], B = dims[1], Cg = dims[2], HW = dims[3], K = dims[4];
    const int rc = pod_sizes(S, B, HW, Cg, K);
    if (rc != 0) return rc;
    if (!plan) return -3;
    const PodPlan g = pod_plan(S, B, Cg, HW);
    plan[0] = g.P;
    plan[1] = g.SL;
    plan[2] = g.L;
    plan[3] = g.ws;
    return 0;
}

extern "C" int tmg_ens_pod_project(const void* rows, const int64_t* t_d, const int64_t* ch, const void* a, const void* m, const void* psi,
                                   void* ws, int64_t ws_floats, void* coef, void* en, const int64_t* o_d, const int64_t* dims,
                                   hipStream_t st) {
    if (!dims) return -3;
    const int64_t k = dims[0], B = dims[1], HW = dims[2], Cg = dims[3], K = dims[4];
    int rc = pod_sizes(k, B, HW, Cg, K);
    if (rc == -1) return rc;
    PodChannels pc = {{0, 0, 0, 0}};
    if (t_d && (t_d[1] < 0 || t_d[0] < t_d[1] + 1)) return -1;
    if (t_d && ch) {
        for (int c = 0; c < Cg; ++c) {
            if (ch[c] < 0 || ch[c] >= t_d[0] - t_d[1]) return -1;
            for (int d = 0; d < c; ++d)
                if (ch[d] == ch[c]) return -1;
            pc.ch[c] = (int)ch[c];
        }
    }
    if (o_d && (o_d[0] < 0 || o_d[1] < 0 || o_d[2] < 0 || o_d[3] < 0)) return -1;
    if (rc != 0) return rc;
    if (t_d && (t_d[0] >= (1ll << 31) || k * B * HW * t_d[0] >= (1ll << 40))) return -2;
    if (o_d && (B * o_d[0] >= (1ll << 40) || k * o_d[1] >= (1ll << 40) || B * o_d[2] >= (1ll << 40) || k * o_d[3] >= (1ll << 40))) return -2;
    const PodPlan g = pod_plan(k, B, Cg, HW);
    if (g.ws >= (1ll << 40)) return -2;
    if (ws_floats < g.ws) return -1;
    if (!rows || !t_d || !ch || !a || !m || !psi || !coef || !en || !o_d) return -3;
    if (g.P > 1 && !ws) return -3;
    const int vec = (HW % 4 == 0 && ((uintptr_t)psi & 15) == 0) ? 1 : 0;
    const float* yr = (const float*)rows + t_d[1];
    const dim3 grid((unsigned)g.P, (unsigned)((k + POD_MT - 1) / POD_MT), (unsigned)B);
#define POD_LAUNCH(NTL_)                                                                                                              \
    hipLaunchKernelGGL((ens_pod_kernel<NTL_>), grid, dim3(256), 0, st, yr, (int)t_d[0], pc, (const float*)a, (const float*)m,         \
                       (const float*)psi, (float*)ws, (float*)coef, (float*)en, (long long)o_d[0], (long long)o_d[1], (long long)o_d[2], \
                       (long long)o_d[3], (int)k, (int)B, (int)HW, (int)Cg, (int)K, (int)g.SL, (int)g.P, vec)
    if (k <= 16) POD_LAUNCH(1);
    else POD_LAUNCH(4);
#undef POD_LAUNCH
    TMG_CHECK_LAUNCH();
    if (g.P > 1) {
        const int64_t n = k * B * (K + 1);
        hipLaunchKernelGGL(ens_pod_fold_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const float*)ws, (float*)coef,
                           (float*)en, (long long)o_d[0], (long long)o_d[1], (long long)o_d[2], (long long)o_d[3], (int)k, (int)B, (int)K,
                           (int)g.P);
        TMG_CHECK_LAUNCH();
    }
    return 0;
}
