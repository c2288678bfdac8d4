// The upper triangle of a Gram matrix G = Z Z^T over the pixels on the fp32 matrix pipe: what the statistics that need one share.  The
// users are the energy score (tmg_gram.hip: Z = the centred members and target of one channel) and the cross-spectral density of the
// spectral POD (tmg_spod.hip: Z = the real and imaginary parts of the rows' Fourier coefficients over the selected channels).  A
// header, compiled into each of those objects with that file's own flags; the kernel in it is static.  One block per plane
// (blockIdx.z), pixel slice (blockIdx.x) and pair of 64-row macro-tiles I <= J (blockIdx.y; DIAG: I == J) writes its partial Gram
// block into the workspace, no atomics.  Written once here:
//   symgram_plan              NT, NP, the floats of a partial, the slices under the workspace cap
//   symgram_tile<DIAG, NTL>   the block's pair I <= J and the live 16-row tiles of each
//   symgram_store<DIAG, NTL>  the end of a block: the hand-over of waves 1..3 and the store of the whole partial
//   symgram_reduce_kernel     P > 1: the P slices' partials added in slice order (fp32); symgram_reduce launches it
//   symgram_at                where G[m][n] lies
//   SYMGRAM_LAUNCH            the diagonal and off-diagonal grids
// The chunk walk with the MFMA loop stays in the user's kernel, between symgram_tile and symgram_store, in the form given below.  It
// was tried as a function template of this header over a row policy (pass count, per-chunk loads, fragment of (side, tile, run)):
// every shape of that seam cost the four-tile CSD instances registers (127 -> 133 VGPRs and 3 -> 2 waves per SIMD on the diagonal
// one, 180 -> 187 on the off-diagonal one), so the loop is kept where the compiler sees it as before.
//
// Layout.  v_mfma_f32_16x16x4_f32 with the lane maps of tmg_tspec.hip: A[i = l & 15][k = l >> 4], B[k = l >> 4][j = l & 15], D column
// l & 15, rows 4 (l >> 4) + 0..3.  A is a 16-row tile of Z and B the transpose of another, so both operands are held the same way: lane
// l has row l & 15 of its tile and pixel group kq = l >> 4.  The sum over the pixels may run in any order as long as A and B of one
// instruction agree on it: a wave takes 64 consecutive pixels at a time, lane (row, kq) owns the 16 CONSECUTIVE pixels kq 16 .. kq 16 +
// 15 of them (64 bytes: four float4 loads on the users' vector paths) and MFMA step s = 0..15 contracts element s of every lane's
// run.  A row's fragment is formed once per 64 pixels and used for every tile pair it is part of; on a diagonal tile pair A and B are
// the same registers.  Rows >= Z and pixels >= HW are never loaded and their lanes hold 0 (the operands come from torch.empty: 0 * NaN
// is NaN); tile pairs without a valid row issue no MFMA.
//
// Sum order, which the tests' rounding counts are derived from (tests/energy_cases.py, tests/spod_cases.py).  The pixels are cut into
// P slices of SL pixels (SL a multiple of 256, the host's choice: symgram_plan).  Inside a slice a block makes the user's passes in
// order (one for the energy score; one per selected channel, in the order given, for the CSD) and, per pass, wave w of the block's 4
// takes the 64-pixel chunks w, w + 4, .. in order; an MFMA is a k-ordered fmaf chain onto its C input, so one accumulator is a chain of
// at most passes SL / 4 fmaf.  Waves 1..3 hand their accumulators over through LDS and wave 0 adds them in wave order (3 additions),
// then the slices are added in slice order (P - 1 additions).  The users' plans report L = passes SL, the fmaf terms of one partial
// (the four waves' chains end to end, >= L / 4 + 3, the longest dependent chain inside a partial), so that L P >= passes HW.  The
// roundings of an entry beside L + P are the user's: those of its operands and of what it does with G.
// No float atomics anywhere: the same inputs give the same bits.
//
// The walk, as both users write it (NTL: the 16-row tiles of a macro-tile that the instance holds, 4, or 1 for Z <= 16).  Nothing in it
// may be indexed by a run-time value and every loop over NTL, the 16 steps and the 4 D registers is fully unrolled, or the instance
// goes to scratch:
//   f32x4 acc[NTL][NTL] = 0
//   per pass, for (pc = slice SL + wave 64; pc < min(HW, (slice + 1) SL); pc += 256), p0 = pc + kq 16:
//     fa[it] = the fragment of row 16 it + (l & 15) of macro-tile I for the run p0 .. p0 + 15, it < NTL
//     per jt < NTL: fb = fa[jt] (DIAG) or the fragment of that row of macro-tile J; per it < NTL with (!DIAG || it <= jt) && it < nti &&
//     jt < ntj: the 16 steps acc[it][jt] = mfma(fa[it][s], fb[s], acc[it][jt])
#pragma once
#include "tmg_common.h"

#define SYMGRAM_MT 64                          // rows of a macro-tile
#define SYMGRAM_PART (SYMGRAM_MT * SYMGRAM_MT) // floats of one partial: [16 tile pairs x 4 D registers][64 lanes]; 256 for one 16-row tile
#define SYMGRAM_CHUNK 64                       // pixels a wave contracts per step
#define SYMGRAM_SLQ 256                        // slice granularity: 4 waves x one chunk
#define SYMGRAM_TARGET_BLOCKS 768              // the grid the slice count aims at: 256 CUs x 3 blocks (48 KB of LDS each)
#define SYMGRAM_WS_CAP (1ll << 24)             // floats of workspace beyond which the slice count is cut (P = 1 may exceed it)

struct SymgramPlan {
    int64_t NT, NP, part, P, SL, ws;
};

// Z rows, `planes` independent Gram matrices (the grid's z), HW pixels per pass
static inline SymgramPlan symgram_plan(int64_t Z, int64_t planes, int64_t HW) {
    SymgramPlan g;
    g.NT = (Z + SYMGRAM_MT - 1) / SYMGRAM_MT;
    g.NP = g.NT * (g.NT + 1) / 2;
    g.part = Z <= 16 ? 256 : SYMGRAM_PART;                                 // one 16-row tile: the small instance
    const int64_t base = planes * g.NP;
    const int64_t maxp = (HW + SYMGRAM_SLQ - 1) / SYMGRAM_SLQ;
    int64_t P = (SYMGRAM_TARGET_BLOCKS + base - 1) / base;
    const int64_t pcap = SYMGRAM_WS_CAP / (base * g.part) - 1;             // P partials and their sum
    if (P > pcap) P = pcap;
    if (P > maxp) P = maxp;
    if (P < 1) P = 1;
    const TmgSlices s = tmg_slices(HW, P, SYMGRAM_SLQ);
    g.SL = s.SL;
    g.P = s.P;
    g.ws = base * g.part * (g.P + (g.P > 1 ? 1 : 0));
    return g;
}

// The block's macro-tile pair I <= J and the live 16-row tiles (>= 1) of each, of the NTL that the instance holds
struct SymgramTile {
    int I, J, nti, ntj;
};

template <bool DIAG, int NTL>
__device__ __forceinline__ SymgramTile symgram_tile(int Z, int NT) {
    int I = blockIdx.y, J = blockIdx.y;
    if (!DIAG) {                                                           // the q-th pair I < J, rows of the upper triangle in order
        int q = blockIdx.y;
        I = 0;
        while (q >= NT - 1 - I) {
            q -= NT - 1 - I;
            ++I;
        }
        J = I + 1 + q;
    }
    return SymgramTile{I, J, min(NTL, (Z - I * SYMGRAM_MT + 15) >> 4), min(NTL, (Z - J * SYMGRAM_MT + 15) >> 4)};
}

// The end of a block: waves 1..3 hand their accumulators over through LDS, wave 0 adds them in wave order and writes every float of the
// block's partial.  ws: the workspace [planes][NP][P][NTL NTL 256]; the plane is blockIdx.z, the slice blockIdx.x.
template <bool DIAG, int NTL>
__device__ __forceinline__ void symgram_store(const f32x4 (&acc)[NTL][NTL], const SymgramTile& tl, float* ws, int P, int NT) {
    __shared__ float red[3][NTL * NTL * 4][64];                            // waves 1..3: [accumulator register][lane]
    const int wave = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int slice = blockIdx.x, plane = blockIdx.z;
    const int I = tl.I, J = tl.J, nti = tl.nti, ntj = tl.ntj;
    if (wave > 0) {
#pragma unroll
        for (int it = 0; it < NTL; ++it)
#pragma unroll
            for (int jt = 0; jt < NTL; ++jt)
                if ((!DIAG || it <= jt) && it < nti && jt < ntj) {
#pragma unroll
                    for (int v = 0; v < 4; ++v) red[wave - 1][(it * NTL + jt) * 4 + v][l] = acc[it][jt][v];
                }
    }
    __syncthreads();
    if (wave == 0) {
        const int pidx = I * NT - I * (I - 1) / 2 + (J - I);
        const int NP = NT * (NT + 1) / 2;
        float* wp = ws + (((size_t)plane * NP + pidx) * P + slice) * (NTL * NTL * 256) + l;
#pragma unroll
        for (int it = 0; it < NTL; ++it)
#pragma unroll
            for (int jt = 0; jt < NTL; ++jt) {
                const bool live = (!DIAG || it <= jt) && it < nti && jt < ntj;
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int a = (it * NTL + jt) * 4 + v;
                    float t = acc[it][jt][v];
                    if (live) t = ((t + red[0][a][l]) + red[1][a][l]) + red[2][a][l];
                    wp[a * 64] = t;                                        // every float of the partial is written: 0 where nothing is live
                }
            }
    }
}

// G[i] = ws[i][0] + ws[i][1] + .. in slice order; i over [planes][NP] partial blocks of `part` floats
static __global__ __launch_bounds__(256) void symgram_reduce_kernel(const float* __restrict__ ws, float* __restrict__ G, int P, int part) {
#pragma clang fp contract(off)
    const size_t blk = blockIdx.x;
    const int e = blockIdx.y * 256 + threadIdx.x;                          // < part
    const float* wp = ws + blk * P * part + e;
    float a = wp[0];
    for (int s = 1; s < P; ++s) a += wp[(size_t)s * part];
    G[blk * part + e] = a;
}

// P > 1: launches the slice reduction behind the partials.  -> G [planes][NP][part]; the caller checks the launch
static inline const float* symgram_reduce(const SymgramPlan& g, int64_t planes, float* ws, hipStream_t st) {
    if (g.P == 1) return ws;
    float* Gs = ws + planes * g.NP * g.P * g.part;
    hipLaunchKernelGGL(symgram_reduce_kernel, dim3((unsigned)(planes * g.NP), (unsigned)(g.part / 256)), dim3(256), 0, st, (const float*)ws, Gs,
                       (int)g.P, (int)g.part);
    return Gs;
}

// offset of G[m][n], m <= n, inside a plane [NP][part]
__device__ __forceinline__ size_t symgram_at(int m, int n, int NT, int part) {
    const int I = m >> 6, J = n >> 6;
    const int pidx = I * NT - I * (I - 1) / 2 + (J - I);
    const int it = (m >> 4) & 3, jt = (n >> 4) & 3, i = m & 15, j = n & 15;
    return (size_t)pidx * part + (size_t)(((it * 4 + jt) * 4 + (i & 3)) * 64 + j + 16 * (i >> 2));
}

// The Gram launches of a plan g over `planes`, once: the diagonal macro-tile pairs (the one-tile instance when the plan says so), then
// the off-diagonal pairs when there is more than one macro-tile.  KERNEL_: the user's template <bool DIAG, int NTL> __global__.
// Returns from the calling function with the error's code when a launch fails.
#define SYMGRAM_LAUNCH(KERNEL_, G_, PLANES_, ST_, ...)                                                                              \
    do {                                                                                                                            \
        const dim3 gd__((unsigned)(G_).P, (unsigned)(G_).NT, (unsigned)(PLANES_));                                                  \
        const dim3 go__((unsigned)(G_).P, (unsigned)((G_).NP - (G_).NT), (unsigned)(PLANES_));                                      \
        if ((G_).part == 256) hipLaunchKernelGGL((KERNEL_<true, 1>), gd__, dim3(256), 0, ST_, __VA_ARGS__);                         \
        else hipLaunchKernelGGL((KERNEL_<true, 4>), gd__, dim3(256), 0, ST_, __VA_ARGS__);                                          \
        TMG_CHECK_LAUNCH();                                                                                                         \
        if ((G_).NT > 1) {                                                                                                          \
            hipLaunchKernelGGL((KERNEL_<false, 4>), go__, dim3(256), 0, ST_, __VA_ARGS__);                                          \
            TMG_CHECK_LAUNCH();                                                                                                     \
        }                                                                                                                           \
    } while (0)
