// Intensity-scale verification of the ensemble's events (tmg_ops.EnsembleIntensityScale / utils.modelPredIntensityScale): at which
// spatial scale the error of an event forecast sits.  An event k is (channel, raw threshold thr[b][k], direction), strict, as in
// tmg_event.hip; a value that compares false (NaN, or an infinity on the wrong side) is in no event.  The device forms, per level
// l = 0 .. L, the sums over the 2^l x 2^l blocks aligned at pixel (0, 0) of squared and multiplied block counts of the members'
// indicators, the target's and the ensemble count; the host turns them into Haar component energies.
// Definitions, layouts and codes: include/tmglow_hip_iscale.h.
//   ens_iscale_zero_kernel    zeroes the step's three tables (and the count, when several groups add to it), launched by the chunk
//                             call with m0 = 0
//   ens_iscale_chunk_kernel   one chunk of k whole members: reads the chunk's NHWC rows directly, (A, X) per member and level, the
//                             per-pixel count cnt, and Cc of the target when m0 = 0
//   ens_iscale_step_kernel    once per kept step: (AN, XN) from cnt and the target
// One block per 64 x 64 tile of one (case, event) plane; the chunk kernel takes the chunk's members in groups of G <= 8, one block per
// tile and group (iscale_group: enough blocks to fill the chip).  It loads as tmg_ens_event_count does, lanes on consecutive pixels
// of a row: wave w owns the rows 16 w .. 16 w + 15 of the tile, a load is 64 consecutive pixels, and the 64-bit lane mask of the
// compare is the row of the member's indicator, kept in LDS (64 words per member); the next member's 16 loads are in flight while the
// current one is compared.  The lane's own bits add up to the count of its 16 pixels, stored in rows: written (m0 = 0) or added to by
// the block when its tile has one group, added atomically onto the zeros of the zeroing launch when it has several (integer adds:
// the order does not show).  After one barrier thread (wave w, lane) owns the 4 x 4 patch at column 32 (w & 1) + 4 (lane & 7), row
// 32 (w >> 1) + 4 (lane >> 3) of the tile, cut out of four row masks: bit 4 r + c of a 16-bit mask is pixel (r, c) of the patch (the
// step kernel, which reads counts, not bits, loads its patch directly).  Levels 0 - 2 are bit
// counts inside the thread (the whole mask, its four 2 x 2 corners, the whole mask again); levels 3, 4, 5 are the sums over the lane
// pairs at xor distance (1, 8), (2, 16), (4, 32), after which every lane of a block holds the block's sum, and the squares and
// products follow the same butterfly over the remaining distances, so that every block is counted once; level 6 adds the four waves'
// totals through LDS.  Per member and tile a sum is at most 4^6 4096 = 2^24: int32 through the wave and LDS, then one 64-bit integer
// global atomic per non-zero entry.  The sums of n reach S^2 2^24: 64-bit from the lane on.  Integer compares and adds only: no
// float arithmetic, no float atomics.  A pixel outside the field is never read (its address is clamped into the field and its bit
// masked off) and never written; its lane stays for every exchange and barrier.  Every register array is indexed by compile-time
// constants in unrolled loops: no scratch.
#include "tmg_common.h"
#include "tmglow_hip_iscale.h"

#define ISC_MAXC 4
#define ISC_MAXK 4
#define ISC_MAXL 6
#define ISC_MAXS 1024
#define ISC_TILE 64
#define ISC_THREADS 256
#define ISC_GROUP 8
#define ISC_FILL 512

struct IscPlan {
    long long tile, ntx, nty, gx, gy, gz, blocks, threads, group, lds, step_lds, member_words, target_words, ens_words;
};

// The members one block takes of a chunk of k members, `planes` = tiles K B blocks per member group: the largest of 8, 4, 2 that still
// gives ISC_FILL blocks, else 2 (a block forms the target's patch once for its members: larger groups read less, smaller ones fill
// the chip), and k itself when that is smaller.
static int64_t iscale_group(int64_t planes, int64_t k) {
    int64_t G = 2;
    for (int64_t c = 4; c <= ISC_GROUP; c <<= 1)
        if (planes * ((k + c - 1) / c) >= ISC_FILL) G = c;
    return G < k ? G : k;
}

// dims = {S, B, H, W, K, L}; -> 0 and the plan, or the code
static int iscale_plan(const int64_t* dims, IscPlan* q) {
    const int64_t S = dims[0], B = dims[1], H = dims[2], W = dims[3], K = dims[4], L = dims[5];
    if (S < 1 || B < 1 || H < 1 || W < 1 || K < 1 || K > ISC_MAXK || L < 1 || L > ISC_MAXL) return -1;
    if (S > ISC_MAXS || B > 65535 || H >= (1ll << 31) || W >= (1ll << 31) || H * W >= (1ll << 31) - 256) return -2;
    const int64_t nty = (H + ISC_TILE - 1) / ISC_TILE, ntx = (W + ISC_TILE - 1) / ISC_TILE;
    // S^2 4^L H_pad W_pad < 2^63: the first factor is at most 2^32, the padded field under 2^45
    if (nty * ntx * ISC_TILE * ISC_TILE > INT64_MAX / (S * S * (1ll << (2 * L)))) return -2;
    q->tile = ISC_TILE;
    q->ntx = ntx;
    q->nty = nty;
    q->gx = ntx * nty;
    q->gy = K;
    q->gz = B;
    q->blocks = q->gx * q->gy * q->gz;
    q->threads = ISC_THREADS;
    q->group = iscale_group(q->blocks, S);
    q->lds = 8 * (ISC_GROUP + 1) * ISC_TILE + 4 * (4 * ISC_GROUP * 6 * 2 + ISC_GROUP * 4 + 4 * 6 + 4);   // rows, part, wtot, opart, owt
    q->step_lds = 8 * (4 * 6 * 2) + 4 * (4 + 4);
    q->member_words = B * K * S * (L + 1) * 2;
    q->target_words = B * K * (L + 1);
    q->ens_words = B * K * (L + 1) * 2;
    return 0;
}

extern "C" int tmg_ens_iscale_plan(const int64_t* dims, int64_t* out) {
    if (!dims) return -3;
    IscPlan q;
    const int rc = iscale_plan(dims, &q);
    if (rc) return rc;
    if (!out) return -3;
    const long long v[14] = {q.tile, q.ntx, q.nty, q.gx, q.gy, q.gz, q.blocks, q.threads, q.group, q.lds, q.step_lds, q.member_words,
                             q.target_words, q.ens_words};
    for (int i = 0; i < 14; ++i) out[i] = v[i];
    return 0;
}

__global__ __launch_bounds__(256) void ens_iscale_zero_kernel(unsigned long long* __restrict__ mem, unsigned long long* __restrict__ tt,
                                                              unsigned long long* __restrict__ ens, int* __restrict__ cnt, long long nm,
                                                              long long nt, long long ne, long long nc) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < nm) mem[i] = 0ull;
    if (i < nt) tt[i] = 0ull;
    if (i < ne) ens[i] = 0ull;
    if (i < nc) cnt[i] = 0;                                                     // (nc = 0 when one block per tile writes the count itself)
}

// The thread's patch: its first pixel, the in-field mask and the clamped pixel offsets of its rows and columns.
struct IscPatch {
    int px, py;
    unsigned vm;        // bit 4 r + c: pixel (py + r, px + c) lies in the field
    int rb[4], cx[4];   // min(py + r, H - 1) W and min(px + c, W - 1): always inside the field
};

__device__ __forceinline__ IscPatch isc_patch(int tile, int ntx, int H, int W) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int ty = tile / ntx, tx = tile - ty * ntx;
    IscPatch p;
    p.px = tx * ISC_TILE + (w & 1) * 32 + (lane & 7) * 4;
    p.py = ty * ISC_TILE + (w >> 1) * 32 + (lane >> 3) * 4;
    p.vm = 0u;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        p.rb[r] = min(p.py + r, H - 1) * W;
        p.cx[r] = min(p.px + r, W - 1);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (p.py + r < H && p.px + c < W) p.vm |= 1u << (4 * r + c);
    return p;
}

// The 16 values of the patch in the plane base (pixel stride ps, the event's channel already added): 16 independent loads.
__device__ __forceinline__ void isc_load(float (&v)[16], const float* __restrict__ base, int ps, const IscPatch& p) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) v[4 * r + c] = base[(size_t)(p.rb[r] + p.cx[c]) * ps];
}

// Their 16-bit event mask, zero outside the field.
__device__ __forceinline__ unsigned isc_bits(const float (&v)[16], const IscPatch& p, float th, int gt) {
    unsigned m = 0u;
#pragma unroll
    for (int i = 0; i < 16; ++i) m |= ((gt ? v[i] > th : v[i] < th) ? 1u : 0u) << i;
    return m & p.vm;
}

__device__ __forceinline__ unsigned isc_mask(const float* __restrict__ base, int ps, const IscPatch& p, float th, int gt) {
    float v[16];
    isc_load(v, base, ps, p);
    return isc_bits(v, p, th, gt);
}

// The 2 x 2 corners of the patch as bit masks: the blocks of level 1.
#define ISC_Q0 0x0033u
#define ISC_Q1 0x00ccu
#define ISC_Q2 0x3300u
#define ISC_Q3 0xcc00u

// The sum of v over the lane pairs at xor distances dx and dy: the next level's block sum, in every lane of the block.
template <typename T>
__device__ __forceinline__ T isc_up(T v, int dx, int dy) {
    v += __shfl_xor(v, dx, 64);
    v += __shfl_xor(v, dy, 64);
    return v;
}

// The loading side of the chunk kernel.  Wave w takes the rows 16 w .. 16 w + 15 of the tile and lane x its column x: a load of one row
// is 64 consecutive pixels, and the compare's 64-bit lane mask IS the row of the member's indicator.  A pixel outside the field is
// never read (its address is clamped into the field) and its bit is masked off.
struct IscRows {
    int gx, gy0;        // the lane's column and the wave's first row in the field
    int cx;             // min(gx, W - 1)
    bool colok;         // gx < W
};

__device__ __forceinline__ void isc_load_rows(float (&v)[16], const float* __restrict__ base, int ps, const IscRows& q, int H, int W) {
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = base[(size_t)(min(q.gy0 + i, H - 1) * W + q.cx) * ps];
}

// The 16 row masks of the wave's rows -> lane i (< 16) returns row i's; bits[i] is this lane's own bit of row i.
__device__ __forceinline__ unsigned long long isc_row_masks(const float (&v)[16], int (&bits)[16], const IscRows& q, int H, float th, int gt) {
    const int lane = threadIdx.x & 63;
    unsigned long long mine = 0ull;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const bool in = q.colok && q.gy0 + i < H && (gt ? v[i] > th : v[i] < th);
        const unsigned long long m = __ballot(in);
        bits[i] = in ? 1 : 0;
        mine = lane == i ? m : mine;
    }
    return mine;
}

// The thread's 4 x 4 patch of a tile kept as 64 row masks: bit 4 r + c is pixel (r, c) of the patch at (row, col) of the tile.
__device__ __forceinline__ unsigned isc_patch_bits(const unsigned long long* rows, int row, int col) {
    unsigned m = 0u;
#pragma unroll
    for (int r = 0; r < 4; ++r) m |= (unsigned)((rows[row + r] >> col) & 15ull) << (4 * r);
    return m;
}

__global__ __launch_bounds__(ISC_THREADS) void ens_iscale_chunk_kernel(const float* __restrict__ y, int ps, const float* __restrict__ tg,
                                                                       int tps, const float* __restrict__ thr, int* __restrict__ cnt,
                                                                       unsigned long long* __restrict__ mem, unsigned long long* __restrict__ tt,
                                                                       int B, int H, int W, int K, int L, int S, int k, int m0, int ntx,
                                                                       int chans, int dirs, int G, int ng) {
    __shared__ unsigned long long rows[ISC_GROUP + 1][ISC_TILE];   // the tile's row masks of the group's members, then of the target
    __shared__ int part[4][ISC_GROUP][6][2];     // per wave, member of the group, level 0..5: (A, X)
    __shared__ int wtot[ISC_GROUP][4];           // per member of the group and wave: the wave's count
    __shared__ int opart[4][6];                  // per wave and level 0..5: the target's squares
    __shared__ int owt[4];                       // per wave: the target's count
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int g = blockIdx.y / K, e = blockIdx.y - g * K, b = blockIdx.z;     // the member group, the event, the case
    const int ch = (chans >> (4 * e)) & 15, gt = (dirs >> e) & 1;
    const size_t hw = (size_t)H * W;
    const float th = thr[(size_t)b * K + e];
    const int ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
    const int g0 = g * G;
    const int gn = k - g0 < G ? k - g0 : G;                                    // 1 <= gn <= G <= ISC_GROUP members: g0 < k by the grid

    // ---- loading: rows of 64 consecutive pixels, row masks into LDS, the lane's own bits into the count
    IscRows q;
    q.gx = tx * ISC_TILE + lane;
    q.gy0 = ty * ISC_TILE + 16 * w;
    q.cx = min(q.gx, W - 1);
    q.colok = q.gx < W;
    const float* yb = y + ((size_t)g0 * B + b) * hw * ps + ch;                 // member g0 + jj at + jj B hw ps
    const size_t ym = (size_t)B * hw * ps;
    float cur[16], nxt[16];
    int bits[16], cn[16];
    isc_load_rows(cur, tg + (size_t)b * hw * tps + ch, tps, q, H, W);
    isc_load_rows(nxt, yb, ps, q, H, W);                                       // the first member's loads fly during the target's work
    {
        const unsigned long long mine = isc_row_masks(cur, bits, q, H, th, gt);
        if (lane < 16) rows[ISC_GROUP][16 * w + lane] = mine;
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) cn[i] = 0;
    for (int jj = 0; jj < gn; ++jj) {
#pragma unroll
        for (int i = 0; i < 16; ++i) cur[i] = nxt[i];
        isc_load_rows(nxt, yb + (size_t)(jj + 1 < gn ? jj + 1 : jj) * ym, ps, q, H, W);   // the next member's loads fly during this one's work
        const unsigned long long mine = isc_row_masks(cur, bits, q, H, th, gt);
        if (lane < 16) rows[jj][16 * w + lane] = mine;
#pragma unroll
        for (int i = 0; i < 16; ++i) cn[i] += bits[i];
    }
    // the count: one group per tile writes (m0 = 0) or adds by itself; several add atomically, onto the zeros of the zeroing launch
#pragma unroll
    for (int i = 0; i < 16; ++i)
        if (q.colok && q.gy0 + i < H) {
            int* cp = cnt + ((size_t)b * K + e) * hw + (size_t)(q.gy0 + i) * W + q.gx;
            if (ng > 1)
                atomicAdd(cp, cn[i]);
            else
                *cp = (m0 > 0 ? *cp : 0) + cn[i];
        }
    __syncthreads();

    // ---- the levels: the thread's 4 x 4 patch of the tile
    const int prow = (w >> 1) * 32 + (lane >> 3) * 4, pcol = (w & 1) * 32 + (lane & 7) * 4;
    const bool one3 = (lane & 9) == 0, one4 = (lane & 27) == 0;     // one lane per block of level 3 / 4 (level 5: lane 0)
    const unsigned om = isc_patch_bits(rows[ISC_GROUP], prow, pcol);
    const int oq0 = __popc(om & ISC_Q0), oq1 = __popc(om & ISC_Q1), oq2 = __popc(om & ISC_Q2), oq3 = __popc(om & ISC_Q3);
    const int o2 = __popc(om);
    const int o3 = isc_up(o2, 1, 8), o4 = isc_up(o3, 2, 16), o5 = isc_up(o4, 4, 32);
    if (m0 == 0 && g == 0) {                                                   // Cc: the step's first chunk, its first group (block-uniform)
        const int c0 = wave_sum(o2), c1 = wave_sum(oq0 * oq0 + oq1 * oq1 + oq2 * oq2 + oq3 * oq3), c2 = wave_sum(o2 * o2);
        const int c3 = wave_sum(one3 ? o3 * o3 : 0), c4 = wave_sum(one4 ? o4 * o4 : 0);
        if (lane == 0) {
            opart[w][0] = c0;
            opart[w][1] = c1;
            opart[w][2] = c2;
            opart[w][3] = c3;
            opart[w][4] = c4;
            opart[w][5] = o5 * o5;
        }
    }
    if (lane == 0) owt[w] = o5;
    for (int jj = 0; jj < gn; ++jj) {
        const unsigned mk = isc_patch_bits(rows[jj], prow, pcol);
        const int q0 = __popc(mk & ISC_Q0), q1 = __popc(mk & ISC_Q1), q2 = __popc(mk & ISC_Q2), q3 = __popc(mk & ISC_Q3);
        const int c2 = __popc(mk);
        const int c3 = isc_up(c2, 1, 8), c4 = isc_up(c3, 2, 16), c5 = isc_up(c4, 4, 32);
        // levels 0 and 1 share a word (a wave's sums are at most 2^10 and 2^12), level 2 holds A and X (at most 2^14 each)
        unsigned a01 = (unsigned)c2 + ((unsigned)(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3) << 11);
        unsigned x01 = (unsigned)__popc(mk & om) + ((unsigned)(q0 * oq0 + q1 * oq1 + q2 * oq2 + q3 * oq3) << 11);
        unsigned ax2 = (unsigned)(c2 * c2) + ((unsigned)(c2 * o2) << 15);
        a01 = wave_sum(a01);
        x01 = wave_sum(x01);
        ax2 = wave_sum(ax2);
        // from level 3 on every lane of a block holds the block's sum: the butterfly goes on over the blocks
        const int a3 = isc_up(isc_up(c3 * c3, 2, 16), 4, 32), x3 = isc_up(isc_up(c3 * o3, 2, 16), 4, 32);
        const int a4 = isc_up(c4 * c4, 4, 32), x4 = isc_up(c4 * o4, 4, 32);
        if (lane == 0) {
            int* pq = &part[w][jj][0][0];
            pq[0] = (int)(a01 & 0x7ffu);
            pq[1] = (int)(x01 & 0x7ffu);
            pq[2] = (int)(a01 >> 11);
            pq[3] = (int)(x01 >> 11);
            pq[4] = (int)(ax2 & 0x7fffu);
            pq[5] = (int)(ax2 >> 15);
            pq[6] = a3;
            pq[7] = x3;
            pq[8] = a4;
            pq[9] = x4;
            pq[10] = c5 * c5;
            pq[11] = c5 * o5;
            wtot[jj][w] = c5;
        }
    }
    __syncthreads();
    const int otot = owt[0] + owt[1] + owt[2] + owt[3];
    if (m0 == 0 && g == 0 && tid >= 128 && tid - 128 <= L) {                   // Cc, level tid - 128
        const int l = tid - 128;
        const int li = l < 6 ? l : 0;
        const int v = l < 6 ? opart[0][li] + opart[1][li] + opart[2][li] + opart[3][li] : otot * otot;
        if (v) atomicAdd(tt + ((size_t)b * K + e) * (L + 1) + l, (unsigned long long)v);
    }
    if (tid < gn * 14) {                                                       // flush the group: (member, level 0..6, A | X), 112 at most
        const int x = tid & 1, r = tid >> 1;
        const int jj = r / 7, l = r - jj * 7;
        if (l <= L) {
            int v;
            if (l < 6) {
                v = part[0][jj][l][x] + part[1][jj][l][x] + part[2][jj][l][x] + part[3][jj][l][x];
            } else {
                const int tot = wtot[jj][0] + wtot[jj][1] + wtot[jj][2] + wtot[jj][3];
                v = tot * (x ? otot : tot);
            }
            if (v) atomicAdd(mem + (((((size_t)b * K + e) * S + (m0 + g0 + jj)) * (L + 1) + l) * 2 + x), (unsigned long long)v);
        }
    }
}

__global__ __launch_bounds__(ISC_THREADS) void ens_iscale_step_kernel(const int* __restrict__ cnt, const float* __restrict__ tg, int tps,
                                                                      const float* __restrict__ thr, unsigned long long* __restrict__ ens,
                                                                      int B, int H, int W, int K, int L, int ntx, int chans, int dirs) {
    __shared__ long long part[4][6][2];          // per wave and level 0..5: (AN, XN)
    __shared__ int wtot[4], owt[4];              // per wave: the count of n and of the target
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int e = blockIdx.y, b = blockIdx.z;
    const int ch = (chans >> (4 * e)) & 15, gt = (dirs >> e) & 1;
    const size_t hw = (size_t)H * W;
    const float th = thr[(size_t)b * K + e];
    const IscPatch p = isc_patch(blockIdx.x, ntx, H, W);
    const bool one3 = (lane & 9) == 0, one4 = (lane & 27) == 0;
    const unsigned om = isc_mask(tg + (size_t)b * hw * tps + ch, tps, p, th, gt);
    const int* cb = cnt + ((size_t)b * K + e) * hw;
    int n[16];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int v = cb[p.rb[r] + p.cx[c]];
            n[4 * r + c] = ((p.vm >> (4 * r + c)) & 1u) ? v : 0;
        }
    long long a0 = 0, x0 = 0, a1 = 0, x1 = 0;
    int n2 = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        a0 += (long long)n[i] * n[i];
        x0 += ((om >> i) & 1u) ? n[i] : 0;
        n2 += n[i];
    }
#pragma unroll
    for (int qy = 0; qy < 2; ++qy)
#pragma unroll
        for (int qx = 0; qx < 2; ++qx) {
            const int i = 8 * qy + 2 * qx;
            const long long s = n[i] + n[i + 1] + n[i + 4] + n[i + 5];
            a1 += s * s;
            x1 += s * __popc(om & (ISC_Q0 << i));
        }
    const int o2 = __popc(om);
    const int o3 = isc_up(o2, 1, 8), o4 = isc_up(o3, 2, 16), o5 = isc_up(o4, 4, 32);
    const int n3 = isc_up(n2, 1, 8), n4 = isc_up(n3, 2, 16), n5 = isc_up(n4, 4, 32);
    a0 = wave_sum(a0);
    x0 = wave_sum(x0);
    a1 = wave_sum(a1);
    x1 = wave_sum(x1);
    const long long a2 = wave_sum((long long)n2 * n2), x2 = wave_sum((long long)n2 * o2);
    const long long a3 = wave_sum(one3 ? (long long)n3 * n3 : 0ll), x3 = wave_sum(one3 ? (long long)n3 * o3 : 0ll);
    const long long a4 = wave_sum(one4 ? (long long)n4 * n4 : 0ll), x4 = wave_sum(one4 ? (long long)n4 * o4 : 0ll);
    if (lane == 0) {
        long long* q = &part[w][0][0];
        q[0] = a0;
        q[1] = x0;
        q[2] = a1;
        q[3] = x1;
        q[4] = a2;
        q[5] = x2;
        q[6] = a3;
        q[7] = x3;
        q[8] = a4;
        q[9] = x4;
        q[10] = (long long)n5 * n5;
        q[11] = (long long)n5 * o5;
        wtot[w] = n5;
        owt[w] = o5;
    }
    __syncthreads();
    if (tid < 14) {
        const int x = tid & 1, l = tid >> 1;
        if (l <= L) {
            long long v;
            if (l < 6) {
                v = part[0][l][x] + part[1][l][x] + part[2][l][x] + part[3][l][x];
            } else {
                const long long tot = (long long)wtot[0] + wtot[1] + wtot[2] + wtot[3];
                v = tot * (x ? (long long)(owt[0] + owt[1] + owt[2] + owt[3]) : tot);
            }
            if (v) atomicAdd(ens + (((size_t)b * K + e) * (L + 1) + l) * 2 + x, (unsigned long long)v);
        }
    }
}

// ev: K x (channel, direction) host integers -> the channels, 4 bits each, and the directions, 1 bit each; or -1
static int iscale_events(const int64_t* ev, int64_t K, int64_t C, int* chans, int* dirs) {
    *chans = 0;
    *dirs = 0;
    for (int64_t e = 0; e < K; ++e) {
        if (ev[2 * e] < 0 || ev[2 * e] > C - 1 || ev[2 * e + 1] < 0 || ev[2 * e + 1] > 1) return -1;
        *chans |= (int)ev[2 * e] << (4 * e);
        *dirs |= (int)ev[2 * e + 1] << e;
    }
    return 0;
}

static int iscale_bad_d(const int64_t* d, int64_t C) { return d && (d[0] < C || d[1] < 0 || d[1] + C > d[0]); }

extern "C" int tmg_ens_iscale_chunk(const void* y, const int64_t* y_d, const void* target, const int64_t* t_d, const void* thr,
                                    const int64_t* ev, void* cnt, void* member, void* target_tab, void* ens, const int64_t* dims,
                                    hipStream_t st) {
    if (!dims) return -3;
    const int64_t k = dims[0], B = dims[1], H = dims[2], W = dims[3], C = dims[4], S = dims[5], m0 = dims[6], K = dims[7], L = dims[8];
    if (C < 2 || C > ISC_MAXC || k < 1 || m0 < 0 || S < 1 || m0 + k > S || K < 1 || K > ISC_MAXK) return -1;
    if (iscale_bad_d(y_d, C) || iscale_bad_d(t_d, C)) return -1;
    int chans = 0, dirs = 0;
    if (ev && iscale_events(ev, K, C, &chans, &dirs)) return -1;
    const int64_t pd[6] = {S, B, H, W, K, L};
    IscPlan q;
    const int rc = iscale_plan(pd, &q);                                        // its -1, then its -2
    if (rc) return rc;
    if (!y_d || !t_d || !ev) return -3;
    const int64_t HW = H * W;
    if (y_d[0] >= (1ll << 31) || t_d[0] >= (1ll << 31) || (k * B) * HW * y_d[0] >= (1ll << 40) || B * HW * t_d[0] >= (1ll << 40)
        || B * K * HW >= (1ll << 40))
        return -2;
    if (!y || !target || !thr || !cnt || !member || !target_tab || !ens) return -3;
    const int64_t G = iscale_group(q.blocks, k), ng = (k + G - 1) / G;
    if (m0 == 0) {
        const int64_t nc = ng > 1 ? B * K * HW : 0, nz = nc > q.member_words ? nc : q.member_words;
        hipLaunchKernelGGL(ens_iscale_zero_kernel, dim3((unsigned)((nz + 255) / 256)), dim3(256), 0, st, (unsigned long long*)member,
                           (unsigned long long*)target_tab, (unsigned long long*)ens, (int*)cnt, q.member_words, q.target_words, q.ens_words,
                           nc);
        TMG_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(ens_iscale_chunk_kernel, dim3((unsigned)q.gx, (unsigned)(q.gy * ng), (unsigned)q.gz), dim3(ISC_THREADS), 0, st,
                       (const float*)y + y_d[1], (int)y_d[0], (const float*)target + t_d[1], (int)t_d[0], (const float*)thr, (int*)cnt,
                       (unsigned long long*)member, (unsigned long long*)target_tab, (int)B, (int)H, (int)W, (int)K, (int)L, (int)S, (int)k,
                       (int)m0, (int)q.ntx, chans, dirs, (int)G, (int)ng);
    TMG_CHECK_LAUNCH();
    return 0;
}

extern "C" int tmg_ens_iscale_step(const void* cnt, const void* target, const int64_t* t_d, const void* thr, const int64_t* ev, void* ens,
                                   const int64_t* dims, hipStream_t st) {
    if (!dims) return -3;
    const int64_t S = dims[0], B = dims[1], H = dims[2], W = dims[3], C = dims[4], K = dims[5], L = dims[6];
    if (C < 2 || C > ISC_MAXC || K < 1 || K > ISC_MAXK) return -1;
    if (iscale_bad_d(t_d, C)) return -1;
    int chans = 0, dirs = 0;
    if (ev && iscale_events(ev, K, C, &chans, &dirs)) return -1;
    const int64_t pd[6] = {S, B, H, W, K, L};
    IscPlan q;
    const int rc = iscale_plan(pd, &q);
    if (rc) return rc;
    if (!t_d || !ev) return -3;
    const int64_t HW = H * W;
    if (t_d[0] >= (1ll << 31) || B * HW * t_d[0] >= (1ll << 40) || B * K * HW >= (1ll << 40)) return -2;
    if (!cnt || !target || !thr || !ens) return -3;
    hipLaunchKernelGGL(ens_iscale_step_kernel, dim3((unsigned)q.gx, (unsigned)q.gy, (unsigned)q.gz), dim3(ISC_THREADS), 0, st,
                       (const int*)cnt, (const float*)target + t_d[1], (int)t_d[0], (const float*)thr, (unsigned long long*)ens, (int)B,
                       (int)H, (int)W, (int)K, (int)L, (int)q.ntx, chans, dirs);
    TMG_CHECK_LAUNCH();
    return 0;
}
