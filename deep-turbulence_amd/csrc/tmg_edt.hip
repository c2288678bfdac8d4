// Distance-map verification of the ensemble (tmg_ops.EnsembleDistance / utils.modelPredDistance): the exact Euclidean distance
// transform of the event sets of the members and of the target, and the integer sums behind the mean error distance, the Hausdorff
// distances, their quantiles and Baddeley's delta.  Definitions, layout and codes: include/tmglow_hip_edt.h.
//   ens_edt_zero_kernel   presets the step's tables, launched by the chunk call with m0 = 0
//   ens_edt_mask_kernel   the chunk's NHWC rows, once for all K events -> one 64-bit word of the indicator per wave, and the set sizes
//   ens_edt_dist_kernel   the squared distance to the set, per pixel; the target's goes to its map, a member's into the sums
//   ens_edt_step_kernel   the step's member sum and the target's fixed-point distance into the int64 time maps
// The transform is separable.  g(i', j), the distance along row i' from column j to the nearest set pixel of that row, comes from
// the row's mask words by count-leading / count-trailing-zero operations; d2(i, j) = min over i' of (i - i')^2 + g(i', j)^2.  One
// block of 256 threads owns a band of 64 rows of a strip of 64 columns of one field (row, case, event): wave w the rows w, w + 4, ..,
// the lanes the 64 columns, 16 pixels per thread in registers.  The source rows come tile by tile (the tile's mask words by one
// coalesced load into LDS, then 64 rows of g as uint16 in LDS, 8 KiB), the band's own tile first, then the tiles above and below it at growing distance; the block stops when no pixel of it can
// still gain from a tile at that distance, (64 (dt - 1) + 1)^2 >= best, and within a tile a pixel walks away from its own row and
// stops at di^2 >= best.  Lanes of a wave are neighbours in one row, so their walks end together.  A field with an empty set (its
// count is 0) is not searched: every distance is INF.  Integer adds, mins, maxes and atomics only: every output is bitwise
// independent of chunking and run.  Every register array is indexed by compile-time constants in unrolled loops: no scratch.
#include <math.h>
#include "tmg_common.h"
#include "tmglow_hip_edt.h"

#define EDT_MAXC 4
#define EDT_MAXK 4
#define EDT_MAXS 1024
#define EDT_MAXHW 4096
#define EDT_TW 64
#define EDT_TH 64
#define EDT_PX 16
#define EDT_THREADS 256
#define EDT_NONE 32768      // g of a row without a set pixel: its square is INF
#define EDT_INF (1 << 30)
#define EDT_MAXCUT 255
#define EDT_PAIR 11

// The distance kernel's static LDS (the source tile's mask words are dynamic, 8 * 64 * strips bytes): a source tile of g, the two histograms, the block's nine sums and two maxima.
struct EdtLds {
    unsigned short g[EDT_TH][EDT_TW];
    int hs[2][256];
    unsigned long long acc[9];
    int hm[2];
};

struct EdtPlan {
    long long tw, th, nsx, nby, gx, gy, gz, blocks, threads, lds, mask_gx, scratch_words, pair_words, hist_words, count_words, map_words;
};

// dims = {S, B, H, W, K, c}; -> 0 and the plan, or the code
static int edt_plan(const int64_t* dims, EdtPlan* q) {
    const int64_t S = dims[0], B = dims[1], H = dims[2], W = dims[3], K = dims[4], c = dims[5];
    if (S < 1 || B < 1 || H < 1 || W < 1 || K < 1 || K > EDT_MAXK || c < 1 || c > EDT_MAXCUT) return -1;
    if (S > EDT_MAXS || B > 65535 || H > EDT_MAXHW || W > EDT_MAXHW || H * W >= (1ll << 31) - 256) return -2;
    q->tw = EDT_TW;
    q->th = EDT_TH;
    q->nsx = (W + EDT_TW - 1) / EDT_TW;
    q->nby = (H + EDT_TH - 1) / EDT_TH;
    q->gx = q->nsx * q->nby * K;
    q->gy = S;
    q->gz = B;
    q->blocks = q->gx * q->gy * q->gz;
    q->threads = EDT_THREADS;
    q->lds = (long long)sizeof(EdtLds) + 8 * EDT_TH * q->nsx;                   // static, and the tile's words (dynamic): <= 42.1 KiB
    q->mask_gx = (H * q->nsx + 3) / 4;
    q->scratch_words = (S + 1) * B * K * H * q->nsx;
    q->pair_words = B * K * S * EDT_PAIR;
    q->hist_words = B * K * S * 2 * (c + 1);
    q->count_words = B * K * (S + 1);
    q->map_words = B * K * H * W;
    return 0;
}

extern "C" int tmg_ens_edt_plan(const int64_t* dims, int64_t* out) {
    if (!dims) return -3;
    EdtPlan q;
    const int rc = edt_plan(dims, &q);
    if (rc) return rc;
    if (!out) return -3;
    const long long v[16] = {q.tw, q.th, q.nsx, q.nby, q.gx, q.gy, q.gz, q.blocks, q.threads, q.lds, q.mask_gx, q.scratch_words,
                             q.pair_words, q.hist_words, q.count_words, q.map_words};
    for (int i = 0; i < 16; ++i) out[i] = v[i];
    return 0;
}

// w(d2) = 256 c from the cutoff on, else floor(256 sqrt(d2)) = isqrt(65536 d2) < 2^16: a float estimate, then integer compares
// until r^2 <= n < (r + 1)^2, so the estimate's rounding does not show (n < 255^2 2^16 < 2^32).
__host__ __device__ __forceinline__ unsigned edt_fixed(int d2, int c) {
    if (d2 >= c * c) return 256u * (unsigned)c;
    const unsigned n = (unsigned)d2 << 16;
    unsigned r = (unsigned)(256.f * sqrtf((float)d2));
    while ((unsigned long long)r * r > n) --r;
    while ((unsigned long long)(r + 1) * (r + 1) <= n) ++r;
    return r;
}

// The host's statement of edt_fixed, for the tests of the fix-up: out[i] = w(d2[i]) for 0 <= d2[i] <= 2^30.
extern "C" int tmg_ens_edt_fixed(const int64_t* d2, int64_t n, int64_t c, int64_t* out) {
    if (n < 0 || c < 1 || c > EDT_MAXCUT) return -1;
    if (!d2 || !out) return -3;
    for (int64_t i = 0; i < n; ++i) {
        if (d2[i] < 0 || d2[i] > EDT_INF) return -1;
    }
    for (int64_t i = 0; i < n; ++i) out[i] = (int64_t)edt_fixed((int)d2[i], (int)c);
    return 0;
}

// pair: 0, with -1 in the two maxima; hist, count, msum: 0
__global__ __launch_bounds__(256) void ens_edt_zero_kernel(long long* __restrict__ pair, long long* __restrict__ hist, int* __restrict__ count,
                                                           int* __restrict__ msum, long long np, long long nh, long long nc, long long nm) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < np) pair[i] = (i % EDT_PAIR) >= 9 ? -1ll : 0ll;
    if (i < nh) hist[i] = 0ll;
    if (i < nc) count[i] = 0;
    if (i < nm) msum[i] = 0;
}

// One wave per 64 consecutive pixels of an image row: the compare's lane mask is one word of the indicator.  Block row r < k is
// member m0 + r of the chunk, block row k (the call with m0 = 0 only) the target.  A pixel beyond W is in no set.
__global__ __launch_bounds__(256) void ens_edt_mask_kernel(const float* __restrict__ y, int ps, const float* __restrict__ tg, int tps,
                                                           const float* __restrict__ thr, unsigned long long* __restrict__ mask,
                                                           int* __restrict__ count, int B, int H, int W, int K, int S, int k, int m0, int NW,
                                                           int chans, int dirs) {
    const int lane = threadIdx.x & 63;
    const int gw = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (gw >= H * NW) return;                                  // whole waves leave
    const int r = blockIdx.y, b = blockIdx.z;
    const bool tgt = r == k;
    const int row = tgt ? S : m0 + r;
    const int i = gw / NW, wj = gw - i * NW;
    const int col = wj * 64 + lane;
    const bool colok = col < W;
    const size_t hw = (size_t)H * W, pix = (size_t)i * W + min(col, W - 1);
    const float* src = tgt ? tg + ((size_t)b * hw + pix) * tps : y + (((size_t)r * B + b) * hw + pix) * ps;
    for (int e = 0; e < K; ++e) {
        const float v = src[(chans >> (4 * e)) & 15];
        const float th = thr[b * K + e];
        const bool in = colok && (((dirs >> e) & 1) ? v > th : v < th);
        const unsigned long long m = __ballot(in);
        if (lane == 0) {
            mask[((((size_t)row * B + b) * K + e) * H + i) * NW + wj] = m;
            if (m) atomicAdd(count + ((size_t)b * K + e) * (S + 1) + row, __popcll(m));
        }
    }
}

// A pixel's walk over the rows r, r + step, .. of the tile in LDS, before rend, the first of them di rows from its own.
__device__ __forceinline__ int edt_walk(unsigned short (*g)[EDT_TW], int lane, int best, int di, int r, int rend, int step) {
    for (; r != rend; r += step, ++di) {
        const int dd = di * di;
        if (dd >= best) break;
        const int gg = g[r][lane];
        best = min(best, dd + gg * gg);
    }
    return best;
}

__global__ __launch_bounds__(EDT_THREADS) void ens_edt_dist_kernel(const unsigned long long* __restrict__ mask, const int* __restrict__ count,
                                                                   int* __restrict__ dO, int* __restrict__ msum,
                                                                   unsigned long long* __restrict__ pair, unsigned long long* __restrict__ hist,
                                                                   int B, int H, int W, int K, int S, int m0, int c, int nsx, int nby, int tgt) {
    __shared__ EdtLds lds;
    extern __shared__ unsigned long long wd[];                 // the source tile's indicator words, EDT_TH rows of nsx
    unsigned short (*g)[EDT_TW] = lds.g;
    int (*hs)[256] = lds.hs;
    unsigned long long* acc = lds.acc;
    int* hm = lds.hm;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int e = blockIdx.x % K, t = blockIdx.x / K;
    const int sx = t % nsx, by = t / nsx;
    const int b = blockIdx.z;
    const int row = tgt ? S : m0 + (int)blockIdx.y;
    const size_t field = (size_t)b * K + e;
    const unsigned long long* mk = mask + (((size_t)row * B + b) * K + e) * H * nsx;
    const int n = count[field * (S + 1) + row];
    const int col = sx * EDT_TW + lane;
    const bool colok = col < W;
    const int i0 = by * EDT_TH + w;                            // the thread's pixels: rows i0 + 4 q of column col

    if (tid < 9) acc[tid] = 0ull;
    if (tid < 2) hm[tid] = -1;
    for (int i = tid; i < 512; i += EDT_THREADS) (&hs[0][0])[i] = 0;

    int best[EDT_PX];
#pragma unroll
    for (int q = 0; q < EDT_PX; ++q) best[q] = EDT_INF;

    if (n > 0) {                                               // block-uniform
        for (int dt = 0; dt < nby; ++dt) {
            if (dt) {                                          // can a row 64 (dt - 1) + 1 away still improve a pixel of the block?
                const int reach = EDT_TH * (dt - 1) + 1;
                int need = 0;
#pragma unroll
                for (int q = 0; q < EDT_PX; ++q) need |= (colok && i0 + 4 * q < H && best[q] > reach * reach) ? 1 : 0;
                if (!__syncthreads_or(need)) break;
            }
            for (int side = 0; side < (dt ? 2 : 1); ++side) {
                const int tt = side ? by + dt : by - dt;
                if (tt < 0 || tt >= nby) continue;             // block-uniform
                const int r0 = tt * EDT_TH;
                const int nr = min(EDT_TH, H - r0);            // the tile's rows inside the field, >= 1
                __syncthreads();                               // the previous tile has been read
                // ---- the tile's words, nr rows of nsx, contiguous in the scratch: one coalesced load, one memory latency per tile
                for (int x = tid; x < nr * nsx; x += EDT_THREADS) wd[x] = mk[(size_t)r0 * nsx + x];
                __syncthreads();
                // ---- g of the tile's rows: wave w the rows 16 w .. 16 w + 15, a row's words wave-uniform (LDS broadcasts)
                for (int rr = 16 * w; rr < 16 * w + 16 && rr < nr; ++rr) {
                    const unsigned long long* wr = wd + rr * nsx;
                    int lpos = -1, rpos = -1;                  // the nearest set column in the words left / right of the strip's
                    for (int j = sx - 1; j >= 0; --j) {
                        const unsigned long long m = wr[j];
                        if (m) { lpos = j * 64 + 63 - __clzll((long long)m); break; }
                    }
                    for (int j = sx + 1; j < nsx; ++j) {
                        const unsigned long long m = wr[j];
                        if (m) { rpos = j * 64 + __ffsll((long long)m) - 1; break; }
                    }
                    const unsigned long long m = wr[sx];
                    const unsigned long long ml = m & (~0ull >> (63 - lane)), mr = m & (~0ull << lane);
                    const int dl = ml ? lane - (63 - __clzll((long long)ml)) : (lpos >= 0 ? col - lpos : EDT_NONE);
                    const int dr = mr ? __ffsll((long long)mr) - 1 - lane : (rpos >= 0 ? rpos - col : EDT_NONE);
                    g[rr][lane] = (unsigned short)min(dl, dr);
                }
                __syncthreads();
                // ---- every pixel walks the tile away from its own row
#pragma unroll
                for (int q = 0; q < EDT_PX; ++q) {
                    const int i = i0 + 4 * q;
                    if (colok && i < H) {
                        int bb = best[q];
                        if (dt == 0) {
                            bb = edt_walk(g, lane, bb, 0, i - r0, -1, -1);
                            bb = edt_walk(g, lane, bb, 1, i - r0 + 1, nr, 1);
                        } else if (side == 0) {
                            bb = edt_walk(g, lane, bb, i - (r0 + nr - 1), nr - 1, -1, -1);
                        } else {
                            bb = edt_walk(g, lane, bb, r0 - i, 0, nr, 1);
                        }
                        best[q] = bb;
                    }
                }
            }
        }
    }
    __syncthreads();                                           // acc, hm and hs are preset

    const size_t hw = (size_t)H * W;
    if (tgt) {
#pragma unroll
        for (int q = 0; q < EDT_PX; ++q) {
            const int i = i0 + 4 * q;
            if (colok && i < H) dO[field * hw + (size_t)i * W + col] = best[q];
        }
        return;
    }

    // ---- a member: the eleven sums, the two histograms, the per-pixel sum
    int nA = 0, nO = 0, nAO = 0, sOA1 = 0, sAO1 = 0, sD1 = 0, hOA = -1, hAO = -1;
    unsigned long long sOA2 = 0ull, sAO2 = 0ull, sD2 = 0ull;
#pragma unroll
    for (int q = 0; q < EDT_PX; ++q) {
        const int i = i0 + 4 * q;
        if (colok && i < H) {
            const size_t p = field * hw + (size_t)i * W + col;
            const int dA = best[q], dT = dO[p];
            const int wA = (int)edt_fixed(dA, c), wT = (int)edt_fixed(dT, c);
            const bool a = dA == 0, o = dT == 0;
            nA += a ? 1 : 0;
            nO += o ? 1 : 0;
            nAO += (a && o) ? 1 : 0;
            if (o) {
                sOA1 += wA;
                sOA2 += (unsigned long long)((long long)wA * wA);
                hOA = max(hOA, dA);
                atomicAdd(&hs[0][wA >> 8], 1);                 // floor(floor(256 x) / 256) = floor(x); 256 c >> 8 = c
            }
            if (a) {
                sAO1 += wT;
                sAO2 += (unsigned long long)((long long)wT * wT);
                hAO = max(hAO, dT);
                atomicAdd(&hs[1][wT >> 8], 1);
            }
            const int df = wA > wT ? wA - wT : wT - wA;
            sD1 += df;
            sD2 += (unsigned long long)((long long)df * df);
            atomicAdd(msum + p, wA);
        }
    }
    const int m = row;
    {
        const int v0 = wave_sum(nA), v1 = wave_sum(nO), v2 = wave_sum(nAO), v3 = wave_sum(sOA1), v5 = wave_sum(sAO1), v7 = wave_sum(sD1);
        const unsigned long long v4 = wave_sum(sOA2), v6 = wave_sum(sAO2), v8 = wave_sum(sD2);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            hOA = max(hOA, __shfl_xor(hOA, o, 64));
            hAO = max(hAO, __shfl_xor(hAO, o, 64));
        }
        if (lane == 0) {
            atomicAdd(&acc[0], (unsigned long long)v0);
            atomicAdd(&acc[1], (unsigned long long)v1);
            atomicAdd(&acc[2], (unsigned long long)v2);
            atomicAdd(&acc[3], (unsigned long long)v3);
            atomicAdd(&acc[4], v4);
            atomicAdd(&acc[5], (unsigned long long)v5);
            atomicAdd(&acc[6], v6);
            atomicAdd(&acc[7], (unsigned long long)v7);
            atomicAdd(&acc[8], v8);
            atomicMax(&hm[0], hOA);
            atomicMax(&hm[1], hAO);
        }
    }
    __syncthreads();
    unsigned long long* pr = pair + (field * S + m) * EDT_PAIR;
    if (tid < 9) {
        if (acc[tid]) atomicAdd(pr + tid, acc[tid]);
    } else if (tid < 11) {
        if (hm[tid - 9] >= 0) atomicMax((long long*)pr + tid, (long long)hm[tid - 9]);
    }
    unsigned long long* hh = hist + (field * S + m) * 2 * (size_t)(c + 1);
    for (int i = tid; i < 2 * (c + 1); i += EDT_THREADS) {
        const int d = i / (c + 1), j = i - d * (c + 1);
        const int v = hs[d][j];
        if (v) atomicAdd(hh + i, (unsigned long long)v);
    }
}

__global__ __launch_bounds__(256) void ens_edt_step_kernel(const int* __restrict__ msum, const int* __restrict__ dO, long long* __restrict__ tmem,
                                                           long long* __restrict__ ttgt, long long n, int c) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        tmem[i] += (long long)msum[i];
        ttgt[i] += (long long)edt_fixed(dO[i], c);
    }
}

// ev: K x (channel, direction) host integers -> the channels, 4 bits each, and the directions, 1 bit each; or -1
static int edt_events(const int64_t* ev, int64_t K, int64_t C, int* chans, int* dirs) {
    *chans = 0;
    *dirs = 0;
    for (int64_t e = 0; e < K; ++e) {
        if (ev[2 * e] < 0 || ev[2 * e] > C - 1 || ev[2 * e + 1] < 0 || ev[2 * e + 1] > 1) return -1;
        *chans |= (int)ev[2 * e] << (4 * e);
        *dirs |= (int)ev[2 * e + 1] << e;
    }
    return 0;
}

static int edt_bad_d(const int64_t* d, int64_t C) { return d && (d[0] < C || d[1] < 0 || d[1] + C > d[0]); }

extern "C" int tmg_ens_edt_chunk(const void* y, const int64_t* y_d, const void* target, const int64_t* t_d, const void* thr, const int64_t* ev,
                                 void* scratch, void* count, void* dmap, void* msum, void* pair, void* hist, const int64_t* dims,
                                 hipStream_t st) {
    if (!dims) return -3;
    const int64_t k = dims[0], B = dims[1], H = dims[2], W = dims[3], C = dims[4], S = dims[5], m0 = dims[6], K = dims[7], c = dims[8];
    if (C < 2 || C > EDT_MAXC || k < 1 || m0 < 0 || S < 1 || m0 + k > S || K < 1 || K > EDT_MAXK) return -1;
    if (edt_bad_d(y_d, C) || edt_bad_d(t_d, C)) return -1;
    int chans = 0, dirs = 0;
    if (ev && edt_events(ev, K, C, &chans, &dirs)) return -1;
    const int64_t pd[6] = {S, B, H, W, K, c};
    EdtPlan q;
    const int rc = edt_plan(pd, &q);                                           // its -1, then its -2
    if (rc) return rc;
    if (!y_d || !t_d || !ev) return -3;
    const int64_t HW = H * W;
    if (y_d[0] >= (1ll << 31) || t_d[0] >= (1ll << 31) || (k * B) * HW * y_d[0] >= (1ll << 40) || B * HW * t_d[0] >= (1ll << 40)
        || q.map_words >= (1ll << 40) || q.scratch_words >= (1ll << 40))
        return -2;
    if (!y || !target || !thr || !scratch || !count || !dmap || !msum || !pair || !hist) return -3;
    if (m0 == 0) {
        int64_t nz = q.pair_words > q.hist_words ? q.pair_words : q.hist_words;
        nz = nz > q.map_words ? nz : q.map_words;                              // count_words < pair_words
        hipLaunchKernelGGL(ens_edt_zero_kernel, dim3((unsigned)((nz + 255) / 256)), dim3(256), 0, st, (long long*)pair, (long long*)hist,
                           (int*)count, (int*)msum, q.pair_words, q.hist_words, q.count_words, q.map_words);
        TMG_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(ens_edt_mask_kernel, dim3((unsigned)q.mask_gx, (unsigned)(k + (m0 == 0 ? 1 : 0)), (unsigned)B), dim3(256), 0, st,
                       (const float*)y + y_d[1], (int)y_d[0], (const float*)target + t_d[1], (int)t_d[0], (const float*)thr,
                       (unsigned long long*)scratch, (int*)count, (int)B, (int)H, (int)W, (int)K, (int)S, (int)k, (int)m0, (int)q.nsx, chans,
                       dirs);
    TMG_CHECK_LAUNCH();
    if (m0 == 0) {                                                             // the target's map, before any member reads it
        hipLaunchKernelGGL(ens_edt_dist_kernel, dim3((unsigned)q.gx, 1u, (unsigned)B), dim3(EDT_THREADS), (unsigned)(8 * EDT_TH * q.nsx), st,
                           (const unsigned long long*)scratch, (const int*)count, (int*)dmap, (int*)msum, (unsigned long long*)pair,
                           (unsigned long long*)hist, (int)B, (int)H, (int)W, (int)K, (int)S, 0, (int)c, (int)q.nsx, (int)q.nby, 1);
        TMG_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(ens_edt_dist_kernel, dim3((unsigned)q.gx, (unsigned)k, (unsigned)B), dim3(EDT_THREADS), (unsigned)(8 * EDT_TH * q.nsx), st,
                       (const unsigned long long*)scratch, (const int*)count, (int*)dmap, (int*)msum, (unsigned long long*)pair,
                       (unsigned long long*)hist, (int)B, (int)H, (int)W, (int)K, (int)S, (int)m0, (int)c, (int)q.nsx, (int)q.nby, 0);
    TMG_CHECK_LAUNCH();
    return 0;
}

extern "C" int tmg_ens_edt_step(const void* msum, const void* dmap, void* tmem, void* ttgt, const int64_t* dims, hipStream_t st) {
    if (!dims) return -3;
    const int64_t B = dims[0], H = dims[1], W = dims[2], K = dims[3], c = dims[4];
    const int64_t pd[6] = {1, B, H, W, K, c};
    EdtPlan q;
    const int rc = edt_plan(pd, &q);
    if (rc) return rc;
    if (q.map_words >= (1ll << 40)) return -2;
    if (!msum || !dmap || !tmem || !ttgt) return -3;
    hipLaunchKernelGGL(ens_edt_step_kernel, dim3((unsigned)((q.map_words + 255) / 256)), dim3(256), 0, st, (const int*)msum, (const int*)dmap,
                       (long long*)tmem, (long long*)ttgt, q.map_words, (int)c);
    TMG_CHECK_LAUNCH();
    return 0;
}
