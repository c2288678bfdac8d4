// Excursion-set morphology of the ensemble (tmg_ops.EnsembleMorphology / utils.modelPredMorphology): the integer counts behind the
// three Minkowski functionals (area, boundary length, Euler characteristic) of the sets {x > thr_j} of a field, for a whole ladder
// of levels j at once.  Per row (the members, then the target), case, field and level: N pixels in, Nh / Nv horizontal / vertical
// pairs with both in, Nq quads with all four in, Nd quads with exactly a diagonal pair in.
// Definitions, layout and codes: include/tmglow_hip_mink.h.
//   ens_mink_zero_kernel    zeroes the step's table, launched by the chunk call with m0 = 0
//   ens_mink_chunk_kernel   one chunk of k whole members (and the target when m0 = 0): reads the chunk's NHWC rows directly
// The counts come from ranks r = #{j : x > thr_j}, so the cost per pixel does not depend on J: with a, b, c, d the ranks of a quad
// (a upper left, b right, c below, d diagonal) the histograms over 0 .. J of a, min(a, b), min(a, c), min(a, b, c, d) summed over
// the bins above j are N, Nh, Nv, Nq, and +1 at max(b, c), -1 at min(a, d) when the latter is larger (or the same with the diagonals
// swapped: at most one holds) summed over the bins up to j is Nd.
// One block per tile of 64 rows x 63 columns, case and group of G <= 4 members (mink_group: 4, 2 or 1, the largest that still gives
// 1024 blocks: the kernel is bound by the length of a block's serial work, not by bytes, so the chip wants many short blocks), all
// fields.  (A block per whole column of tiles, with a quarter of the blocks and of the global atomics, took 2.5 times as long:
// LAB_NOTES.md.)  Wave w loads the rows 16 w .. 16 w + 16 of the tile, lanes on the 64 consecutive pixels of a row; the 17th row and
// the 64th lane are the halo, owned by the next wave or tile, so each pixel, pair and quad is counted exactly once.  The rank is a
// binary search in the ladder, which the block sorts into LDS first (the rank does not depend on the ladder's order); the right
// neighbour's rank is a lane exchange, the lower one's the lane's next register.  A lane walks down its column with (bins, count) of
// the four histograms in registers, the four bins packed into one key (they change together on smooth fields), and adds to LDS only
// when the key changes and after its last row (a wave whose lanes all hold one key adds once): on smooth fields, where all lanes of
// a wave would hit one LDS word, that is one atomic per wave and 16 rows, not 64 lanes deep per row.  The next (member, field)'s 17
// loads are in flight while the current one is counted.  A bin holds at most 64 * 63 per row and field: int32 through LDS, then one
// 64-bit integer global atomic per non-zero entry.  Integer compares, min, max and adds only.  A pixel outside the field is never
// read (its address is clamped into the field, its rank 0) and its lane stays for every exchange and barrier.  Every register array
// is indexed by compile-time constants in unrolled loops: no scratch.
#include "tmg_common.h"
#include "tmglow_hip_mink.h"

#define MNK_MAXC 4
#define MNK_MAXF 4
#define MNK_MAXJ 32
#define MNK_MAXS 1024
#define MNK_TH 64
#define MNK_TW 63
#define MNK_ROWS 16
#define MNK_THREADS 256
#define MNK_GROUP 4
#define MNK_FILL 1024
#define MNK_BINS (MNK_MAXJ + 1)
#define MNK_LADDER (MNK_MAXJ + 2)

struct MnkPlan {
    long long th, tw, ntx, nty, gx, gy, gz, blocks, threads, group, lds, table_words;
};

// The members one block takes of a chunk of k members, `planes` = tiles B blocks per member group: the largest of 4, 2 that still
// gives MNK_FILL blocks, else 1 (a block sorts the ladders and sums the histograms once for its members, but its members are serial
// work: many short blocks fill the chip), and k itself when that is smaller.
static int64_t mink_group(int64_t planes, int64_t k) {
    int64_t G = 1;
    for (int64_t c = 2; c <= MNK_GROUP; c <<= 1)
        if (planes * ((k + c - 1) / c) >= MNK_FILL) G = c;
    return G < k ? G : k;
}

// dims = {S, B, H, W, F, J}; -> 0 and the plan, or the code
static int mink_plan(const int64_t* dims, MnkPlan* q) {
    const int64_t S = dims[0], B = dims[1], H = dims[2], W = dims[3], F = dims[4], J = dims[5];
    if (S < 1 || B < 1 || H < 1 || W < 1 || F < 1 || F > MNK_MAXF || J < 1 || J > MNK_MAXJ) return -1;
    if (S > MNK_MAXS || B > 65535 || H >= (1ll << 31) || W >= (1ll << 31) || H * W >= (1ll << 31) - 256) return -2;
    q->th = MNK_TH;
    q->tw = MNK_TW;
    q->ntx = (W + MNK_TW - 1) / MNK_TW;
    q->nty = (H + MNK_TH - 1) / MNK_TH;
    q->gx = q->ntx * q->nty;
    q->gz = B;
    q->group = mink_group(q->gx * q->gz, S);
    q->gy = (S + q->group - 1) / q->group + 1;
    q->blocks = q->gx * q->gy * q->gz;
    q->threads = MNK_THREADS;
    q->lds = 4 * (MNK_GROUP * MNK_MAXF * 5 * MNK_BINS) + 4 * (MNK_MAXF * MNK_LADDER) + 4 * (MNK_MAXF * MNK_MAXJ);   // hist, sl, raw
    q->table_words = B * F * (S + 1) * J * 5;
    return 0;
}

extern "C" int tmg_ens_mink_plan(const int64_t* dims, int64_t* out) {
    if (!dims) return -3;
    MnkPlan q;
    const int rc = mink_plan(dims, &q);
    if (rc) return rc;
    if (!out) return -3;
    const long long v[12] = {q.th, q.tw, q.ntx, q.nty, q.gx, q.gy, q.gz, q.blocks, q.threads, q.group, q.lds, q.table_words};
    for (int i = 0; i < 12; ++i) out[i] = v[i];
    return 0;
}

__global__ __launch_bounds__(256) void ens_mink_zero_kernel(unsigned long long* __restrict__ table, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) table[i] = 0ull;
}

// The wave's 17 rows of one plane (pixel stride ps, the field's channel already added): 17 independent loads of 64 consecutive pixels.
__device__ __forceinline__ void mnk_load_rows(float (&v)[MNK_ROWS + 1], const float* __restrict__ base, int ps, int gy0, int cx, int H, int W) {
#pragma unroll
    for (int i = 0; i <= MNK_ROWS; ++i) v[i] = base[(size_t)(min(gy0 + i, H - 1) * W + cx) * ps];
}

// #{j : x > thr_j} by binary search in the sorted ladder s[0 .. 31] (+Inf from J on): x > s[i] holds exactly for i < rank.  The five
// steps find min(rank, 31), the last one tells 31 from 32.  NaN compares false everywhere: rank 0.
// (Walking a pointer, not an index: a step is one LDS read at a constant offset, a compare, a select and an add.)
__device__ __forceinline__ int mnk_rank(float x, const float* s) {
    const float* p = s;
#pragma unroll
    for (int st = 16; st > 0; st >>= 1) p += x > p[st - 1] ? st : 0;
    return (int)(p - s) + (x > *p ? 1 : 0);
}

// The four bins of a pixel travel as one key, a | min(a,b) << 8 | min(a,c) << 16 | min(a,b,c,d) << 24: on smooth fields the four change
// together or not at all, so one run of equal keys down the lane's column stands for the runs of all four histograms.  A finished
// run of cc pixels goes to LDS; bin 0 takes what is in no set and is never read.
__device__ __forceinline__ void mnk_add4(int* h, unsigned key, int cc) {
    atomicAdd(h + (key & 255u), cc);
    atomicAdd(h + MNK_BINS + ((key >> 8) & 255u), cc);
    atomicAdd(h + 2 * MNK_BINS + ((key >> 16) & 255u), cc);
    atomicAdd(h + 3 * MNK_BINS + (key >> 24), cc);
}

// The last run of the column.  Where all lanes of the wave hold one key (a smooth field) the wave adds once.  Called by whole waves.
__device__ __forceinline__ void mnk_flush(int* h, unsigned ck, int cc) {
    const unsigned first = (unsigned)__builtin_amdgcn_readfirstlane((int)ck);
    if (__all(ck == first)) {
        const int s = wave_sum(cc);
        if ((threadIdx.x & 63) == 0 && first) mnk_add4(h, first, s);
    } else if (ck) {
        mnk_add4(h, ck, cc);
    }
}

__global__ __launch_bounds__(MNK_THREADS) void ens_mink_chunk_kernel(const float* __restrict__ y, int ps, const float* __restrict__ tg, int tps,
                                                                     const float* __restrict__ thr, unsigned long long* __restrict__ table,
                                                                     int B, int H, int W, int F, int J, int S, int k, int m0, int ntx,
                                                                     int chans, int G, int ng) {
    __shared__ int hist[MNK_GROUP][MNK_MAXF][5][MNK_BINS];   // per member of the group and field: a, min(a,b), min(a,c), min(a,b,c,d), diagonal
    __shared__ float sl[MNK_MAXF][MNK_LADDER];               // per field: the sorted ladder, +Inf from J on
    __shared__ float raw[MNK_MAXF][MNK_MAXJ];                // per field: the ladder as given, padded
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int g = blockIdx.y, b = blockIdx.z;
    const bool tgt = g == ng;                                // the target's block row (m0 = 0 only), block-uniform
    const int g0 = tgt ? 0 : g * G;
    const int gn = tgt ? 1 : (k - g0 < G ? k - g0 : G);      // 1 <= gn <= G <= MNK_GROUP: g0 < k by the grid
    const size_t hw = (size_t)H * W;
    const float inf = __builtin_huge_valf();

    for (int i = tid; i < MNK_GROUP * MNK_MAXF * 5 * MNK_BINS; i += MNK_THREADS) (&hist[0][0][0][0])[i] = 0;
    // the ladders: one global read per level into LDS (padded to 32 with +Inf; NaN counts as +Inf), then a rank sort out of LDS
    float v = inf;
    if (tid < 32 * F) {
        const int f = tid >> 5, j = tid & 31;
        if (j < J) v = thr[((size_t)b * F + f) * J + j];
        v = v == v ? v : inf;
        raw[f][j] = v;
    }
    __syncthreads();
    if (tid < 32 * F) {
        const int f = tid >> 5, j = tid & 31;
        int pos = 0;
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            const float u = raw[f][i];
            pos += (u < v || (u == v && i < j)) ? 1 : 0;
        }
        sl[f][pos] = v;
        if (j < 2) sl[f][32 + j] = inf;
    }
    __syncthreads();

    const int ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
    const int gx = tx * MNK_TW + lane, gy0 = ty * MNK_TH + MNK_ROWS * w;
    const int cx = min(gx, W - 1);
    const bool colok = gx < W, own = lane < MNK_TW;
    const int sps = tgt ? tps : ps;
    const float* sb = tgt ? tg + (size_t)b * hw * tps : y + ((size_t)g0 * B + b) * hw * ps;     // member g0 + jj at + jj B hw ps
    const size_t ym = (size_t)B * hw * ps;
    const int nit = gn * F;
    float cur[MNK_ROWS + 1], nxt[MNK_ROWS + 1];
    mnk_load_rows(nxt, sb + (chans & 15), sps, gy0, cx, H, W);
    for (int it = 0; it < nit; ++it) {
        const int jj = it / F, f = it - jj * F;
#pragma unroll
        for (int i = 0; i <= MNK_ROWS; ++i) cur[i] = nxt[i];
        {
            const int in = it + 1 < nit ? it + 1 : it;       // the next (member, field)'s loads fly during this one's work
            const int nj = in / F, nf = in - nj * F;
            mnk_load_rows(nxt, sb + (size_t)nj * ym + ((chans >> (4 * nf)) & 15), sps, gy0, cx, H, W);
        }
        const float* s = sl[f];
        int r[MNK_ROWS + 1], rr[MNK_ROWS + 1];
#pragma unroll
        for (int i = 0; i <= MNK_ROWS; ++i) {
            const int q = mnk_rank(cur[i], s);
            const int v = (colok && gy0 + i < H) ? q : 0;
            rr[i] = __shfl_down(v, 1, 64);                   // the right neighbour's (lane 63: its own, never used)
            r[i] = own ? v : 0;                              // the halo column counts nothing of its own
            rr[i] = own ? rr[i] : 0;
        }
        int* h = &hist[jj][f][0][0];
        unsigned ck = 0u;
        int cc = 0;
#pragma unroll
        for (int i = 0; i < MNK_ROWS; ++i) {
            const int a = r[i], bb = rr[i], c = r[i + 1], d = rr[i + 1];
            const int m1 = min(a, bb), m2 = min(a, c), m3 = min(m1, min(c, d));
            const unsigned key = (unsigned)a | ((unsigned)m1 << 8) | ((unsigned)m2 << 16) | ((unsigned)m3 << 24);
            if (key != ck) {                                 // the run ends here; a run of zeros counts nothing
                if (ck) mnk_add4(h, ck, cc);
                ck = key;
                cc = 0;
            }
            ++cc;
            const int lo1 = max(bb, c), hi1 = min(a, d), lo2 = max(a, d), hi2 = min(bb, c);
            const bool one = hi1 > lo1;
            const int lo = one ? lo1 : lo2, hi = one ? hi1 : hi2;
            if (hi > lo) {                                   // a diagonal pair of the levels lo .. hi - 1
                atomicAdd(h + 4 * MNK_BINS + lo, 1);
                atomicAdd(h + 4 * MNK_BINS + hi, -1);
            }
        }
        mnk_flush(h, ck, cc);
    }
    __syncthreads();

    // ---- the sums over the bins above j (below and at j for the diagonal pairs): one entry per thread and turn
    const int ne = gn * F * J * 5;
    for (int e = tid; e < ne; e += MNK_THREADS) {
        const int q = e % 5, e1 = e / 5;
        const int j = e1 % J, e2 = e1 / J;
        const int f = e2 % F, jj = e2 / F;
        const int* hh = hist[jj][f][q];
        int v = 0;
        if (q < 4)
            for (int i = j + 1; i <= J; ++i) v += hh[i];
        else
            for (int i = 0; i <= j; ++i) v += hh[i];
        const int row = tgt ? S : m0 + g0 + jj;
        if (v) atomicAdd(table + ((((size_t)b * F + f) * (S + 1) + row) * J + j) * 5 + q, (unsigned long long)v);
    }
}

// fields: F host integers, distinct channels in 0 .. C - 1 -> the channels, 4 bits each; or -1
static int mink_fields(const int64_t* fields, int64_t F, int64_t C, int* chans) {
    *chans = 0;
    int seen = 0;
    for (int64_t f = 0; f < F; ++f) {
        if (fields[f] < 0 || fields[f] > C - 1 || ((seen >> fields[f]) & 1)) return -1;
        seen |= 1 << fields[f];
        *chans |= (int)fields[f] << (4 * f);
    }
    return 0;
}

static int mink_bad_d(const int64_t* d, int64_t C) { return d && (d[0] < C || d[1] < 0 || d[1] + C > d[0]); }

extern "C" int tmg_ens_mink_chunk(const void* y, const int64_t* y_d, const void* target, const int64_t* t_d, const void* thr,
                                  const int64_t* fields, void* table, const int64_t* dims, hipStream_t st) {
    if (!dims) return -3;
    const int64_t k = dims[0], B = dims[1], H = dims[2], W = dims[3], C = dims[4], S = dims[5], m0 = dims[6], F = dims[7], J = dims[8];
    if (C < 2 || C > MNK_MAXC || k < 1 || m0 < 0 || S < 1 || m0 + k > S || F < 1 || F > MNK_MAXF) return -1;
    if (mink_bad_d(y_d, C) || mink_bad_d(t_d, C)) return -1;
    int chans = 0;
    if (fields && mink_fields(fields, F, C, &chans)) return -1;
    const int64_t pd[6] = {S, B, H, W, F, J};
    MnkPlan q;
    const int rc = mink_plan(pd, &q);                                          // its -1, then its -2
    if (rc) return rc;
    if (!y_d || !t_d || !fields) return -3;
    const int64_t HW = H * W;
    if (y_d[0] >= (1ll << 31) || t_d[0] >= (1ll << 31) || (k * B) * HW * y_d[0] >= (1ll << 40) || B * HW * t_d[0] >= (1ll << 40)) return -2;
    if (!y || !target || !thr || !table) return -3;
    const int64_t G = mink_group(q.gx * q.gz, k), ng = (k + G - 1) / G;
    if (m0 == 0) {
        hipLaunchKernelGGL(ens_mink_zero_kernel, dim3((unsigned)((q.table_words + 255) / 256)), dim3(256), 0, st, (unsigned long long*)table,
                           q.table_words);
        TMG_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(ens_mink_chunk_kernel, dim3((unsigned)q.gx, (unsigned)(ng + (m0 == 0 ? 1 : 0)), (unsigned)q.gz), dim3(MNK_THREADS), 0, st,
                       (const float*)y + y_d[1], (int)y_d[0], (const float*)target + t_d[1], (int)t_d[0], (const float*)thr,
                       (unsigned long long*)table, (int)B, (int)H, (int)W, (int)F, (int)J, (int)S, (int)k, (int)m0, (int)q.ntx, chans, (int)G,
                       (int)ng);
    TMG_CHECK_LAUNCH();
    return 0;
}
