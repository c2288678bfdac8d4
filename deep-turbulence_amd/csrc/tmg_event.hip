// Probabilistic event verification of sampled roll-outs against the target (tmg_ops.EnsembleEvents / utils.modelPredEvents).  An event
// k is (channel, raw threshold thr[b][k], direction), strict.  Per pixel p: n = #{m : x_m <> thr} over the S raw normalised members
// (0..S), o = [y <> thr] of the raw normalised target.  Everything the device forms is an integer:
//   rel_count[j] = #{p : n = j}, rel_hit[j] = #{p : n = j, o = 1}                         the reliability tables, S + 1 bins
//   A = sum_p Nf^2, Bx = sum_p Nf No, Cc = sum_p No^2 per neighbourhood width w           the raw sums of the fractions skill score,
//       Nf(p) / No(p) = the sum of n / o over the w x w box centred on p, zeros outside the field
//   sum_t n, sum_t o, sum_t n^2, sum_t n o per pixel                                      the running sums over the timed steps
//   ens_event_count_kernel   one chunk of k whole members: reads the chunk's NHWC rows directly and folds them into the planar
//                            counts cnt [B][K][HW] (m0 = 0 writes, later chunks add): no member buffer, O(B K HW) device memory
//   ens_event_zero_kernel    zeroes the step's own table and raw-sum planes
//   ens_event_step_kernel    once per kept step, after the step's last chunk: one block per 32 x 32 tile of one (case, event) plane
// Integer adds only (LDS int32 atomics, then one global int32 add per non-empty bin and block; 64-bit integer adds for the raw sums):
// their sums do not depend on the order, so every output is bitwise reproducible.  No float atomics, no float arithmetic at all.
//
// The step kernel.  A block loads its tile plus a halo of R = max w / 2 pixels of n (from cnt) and of o (formed from the target on the
// fly) into two LDS tables of (TH + 2 R + 1) rows of `pitch` ints, entry (y + 1, x + 1), row 0 and column 0 zero; pixels outside the
// field are zero.  While loading, the thread that holds a pixel of the tile itself counts it into the block's LDS histograms and
// advances the pixel's four time sums.  Then the tables become tile-local summed-area tables in place: a row pass (one thread per
// row of one table, lanes on consecutive rows) and a column pass (one thread per column, lanes on consecutive columns).  Every box
// sum of every width is then four reads: T[y1][x1] - T[y0][x1] - T[y1][x0] + T[y0][x0]; the halo holds every box of the tile whole,
// so the cost does not depend on the number or the size of the widths.  A table entry is at most 64 * 64 * 1024 < 2^23.
// LDS banks are (a / 4) mod 32.  The column pass and the evaluation have lanes on consecutive columns: consecutive banks at any pitch.
// The row pass has lanes on consecutive rows, stride `pitch` ints: pitch is made odd (TW + 2 R + 1 is), so 32 consecutive rows fall
// on 32 different banks; an even pitch of 64 would put the whole wave on one bank.
// Every thread owns 4 pixels of the tile and EVENT_MAXNS x 3 int64 accumulators, indexed by compile-time constants in unrolled loops
// (no scratch); they are added over the wave (shuffles), over the block's 4 waves (LDS) and across the tiles (one 64-bit integer
// atomic add per sum and block into the zeroed output).
#include "tmg_common.h"
#include "tmglow_hip.h"

#define EVENT_MAXC 4
#define EVENT_MAXK 4
#define EVENT_MAXNS 8
#define EVENT_MAXW 33
#define EVENT_MAXS 1024
#define EVENT_T 32           // tile height and width
#define EVENT_THREADS 256

struct EventArgs {
    int ech[EVENT_MAXK];     // the events' channels
    int egt[EVENT_MAXK];     // 1: x > thr, 0: x < thr
    int r[EVENT_MAXNS];      // w / 2 of every width
};

struct EventPlan {
    long long th, tw, halo, nty, ntx, lds, threads, ws, pitch, rows, blocks, sat_ints;
};

// dims = {S, B, H, W, K, NS}; -> 0 and the plan, or the code
static int event_plan(const int64_t* dims, const int64_t* scales, EventPlan* q) {
    const int64_t S = dims[0], B = dims[1], H = dims[2], W = dims[3], K = dims[4], NS = dims[5];
    if (S < 1 || B < 1 || H < 1 || W < 1 || K < 1 || K > EVENT_MAXK || NS < 1 || NS > EVENT_MAXNS) return -1;
    int64_t wmax = 1;
    for (int64_t i = 0; scales && i < NS; ++i) {                               // (a null list is the caller's -3, after the sizes)
        const int64_t w = scales[i];
        if (w < 1 || w > EVENT_MAXW || !(w & 1)) return -1;
        for (int64_t j = 0; j < i; ++j)
            if (scales[j] == w) return -1;
        wmax = w > wmax ? w : wmax;
    }
    if (S > EVENT_MAXS || B > 65535 || H >= (1ll << 31) || W >= (1ll << 31) || H * W >= (1ll << 31) - 256) return -2;
    // the int64 raw sums: S^2 w^4 HW < 2^63
    const unsigned __int128 top = (unsigned __int128)(S * S) * (unsigned __int128)(wmax * wmax * wmax * wmax) * (unsigned __int128)(H * W);
    if (top >= ((unsigned __int128)1 << 63)) return -2;
    q->th = q->tw = EVENT_T;
    q->halo = wmax / 2;
    q->nty = (H + EVENT_T - 1) / EVENT_T;
    q->ntx = (W + EVENT_T - 1) / EVENT_T;
    q->rows = EVENT_T + 2 * q->halo + 1;
    q->pitch = EVENT_T + 2 * q->halo + 1;                                      // odd: see the header
    q->sat_ints = q->rows * q->pitch;
    // two tables, the two histograms of S + 1 bins, then 4 waves x 24 int64 of the block reduction (at an even number of ints)
    q->lds = 4 * (2 * q->sat_ints + 2 * (S + 1)) + 8 * 4 * 3 * EVENT_MAXNS;
    q->threads = EVENT_THREADS;
    q->ws = 0;
    q->blocks = q->nty * q->ntx * K * B;
    if (q->nty * q->ntx >= (1ll << 31)) return -2;
    return 0;
}

extern "C" int tmg_ens_event_plan(const int64_t* dims, const int64_t* scales, int64_t* plan) {
    if (!dims) return -3;
    EventPlan q;
    const int rc = event_plan(dims, scales, &q);
    if (rc) return rc;
    if (!scales || !plan) return -3;
    const long long v[12] = {q.th, q.tw, q.halo, q.nty, q.ntx, q.lds, q.threads, q.ws, q.pitch, q.rows, q.blocks, 0};
    for (int i = 0; i < 12; ++i) plan[i] = v[i];
    return 0;
}

__global__ __launch_bounds__(256) void ens_event_count_kernel(const float* __restrict__ y, int ps, const float* __restrict__ thr,
                                                              int* __restrict__ cnt, int B, int HW, int K, int k, int m0, EventArgs a) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    if (p >= HW) return;
    const size_t hw = (size_t)HW;
    float th[EVENT_MAXK];
    int c[EVENT_MAXK];
#pragma unroll
    for (int e = 0; e < EVENT_MAXK; ++e) {
        th[e] = e < K ? thr[(size_t)b * K + e] : 0.f;
        c[e] = 0;
    }
    for (int j = 0; j < k; ++j) {
        const float* yp = y + ((size_t)(j * B + b) * hw + p) * ps;
#pragma unroll
        for (int e = 0; e < EVENT_MAXK; ++e) {
            if (e < K) {
                const float v = yp[a.ech[e]];
                c[e] += (a.egt[e] ? v > th[e] : v < th[e]) ? 1 : 0;
            }
        }
    }
#pragma unroll
    for (int e = 0; e < EVENT_MAXK; ++e) {
        if (e < K) {
            int* cp = cnt + ((size_t)b * K + e) * hw + p;
            *cp = (m0 > 0 ? *cp : 0) + c[e];
        }
    }
}

// ev: K x (channel, direction) host integers -> the kernel's argument block, or -1
static int event_args(const int64_t* ev, int64_t K, int64_t C, EventArgs* a) {
    for (int e = 0; e < EVENT_MAXK; ++e) {
        a->ech[e] = 0;
        a->egt[e] = 0;
    }
    for (int64_t e = 0; e < K; ++e) {
        if (ev[2 * e] < 0 || ev[2 * e] > C - 1 || ev[2 * e + 1] < 0 || ev[2 * e + 1] > 1) return -1;
        a->ech[e] = (int)ev[2 * e];
        a->egt[e] = (int)ev[2 * e + 1];
    }
    return 0;
}

extern "C" int tmg_ens_event_count(const void* y, const int64_t* y_d, const void* thr, const int64_t* ev, void* cnt, const int64_t* dims,
                                   hipStream_t st) {
    if (!dims) return -3;
    const int64_t k = dims[0], B = dims[1], HW = dims[2], C = dims[3], S = dims[4], m0 = dims[5], K = dims[6];
    if (k < 1 || B < 1 || HW < 1 || C < 2 || C > EVENT_MAXC || S < 1 || m0 < 0 || m0 + k > S || K < 1 || K > EVENT_MAXK) return -1;
    if (y_d && (y_d[0] < C || y_d[1] < 0 || y_d[1] + C > y_d[0])) return -1;
    EventArgs a;
    if (ev && event_args(ev, K, C, &a)) return -1;
    if (!y_d || !ev) return -3;
    if (S > EVENT_MAXS || HW >= (1ll << 31) - 256 || B > 65535 || y_d[0] >= (1ll << 31)) return -2;
    if ((k * B) * HW * y_d[0] >= (1ll << 40) || B * K * HW >= (1ll << 40)) return -2;
    if (!y || !thr || !cnt) return -3;
    for (int i = 0; i < EVENT_MAXNS; ++i) a.r[i] = 0;
    dim3 grid((unsigned)((HW + 255) / 256), (unsigned)B);
    hipLaunchKernelGGL(ens_event_count_kernel, grid, dim3(256), 0, st, (const float*)y + y_d[1], (int)y_d[0], (const float*)thr, (int*)cnt,
                       (int)B, (int)HW, (int)K, (int)k, (int)m0, a);
    TMG_CHECK_LAUNCH();
    return 0;
}

__global__ __launch_bounds__(256) void ens_event_zero_kernel(int* __restrict__ rcnt, int* __restrict__ rhit, long long* __restrict__ fss,
                                                             long long rcs, long long fcs, int nrel, int nfss) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < nrel) {
        rcnt[(size_t)b * rcs + i] = 0;
        rhit[(size_t)b * rcs + i] = 0;
    }
    if (i < nfss) fss[(size_t)b * fcs + i] = 0;
}

__global__ __launch_bounds__(EVENT_THREADS) void ens_event_step_kernel(const int* __restrict__ cnt, const float* __restrict__ tgt, int tps,
                                                                       const float* __restrict__ thr, int* __restrict__ rcnt,
                                                                       int* __restrict__ rhit, long long* __restrict__ fss,
                                                                       int* __restrict__ tsum, long long rcs, long long fcs, int S, int B,
                                                                       int H, int W, int K, int NS, int R, int ntx, int t_before, int flags,
                                                                       EventArgs a) {
    extern __shared__ int lds[];
    const int tid = threadIdx.x;
    const int k = blockIdx.y, b = blockIdx.z;
    const int ty0 = (blockIdx.x / ntx) * EVENT_T, tx0 = (blockIdx.x % ntx) * EVENT_T;
    const int RW = EVENT_T + 2 * R;                                            // the region's width and height (tile plus halo)
    const int pitch = RW + 1, rows = RW + 1;
    const int sat = rows * pitch;
    int* Tn = lds;
    int* To = lds + sat;
    int* bins = lds + 2 * sat;                                                 // [2][S + 1]
    long long* red = (long long*)(lds + 2 * sat + 2 * (S + 1));                // an even number of ints: 8-byte aligned
    const size_t hw = (size_t)H * W;
    int ch = 0, gt = 0;
#pragma unroll
    for (int e = 0; e < EVENT_MAXK; ++e) {                                     // (constant indices: the argument block stays in SGPRs)
        if (e == k) {
            ch = a.ech[e];
            gt = a.egt[e];
        }
    }
    const float th = thr[(size_t)b * K + k];
    const int* cp = cnt + ((size_t)b * K + k) * hw;
    const float* tp = tgt + (size_t)b * hw * tps + ch;

    for (int i = tid; i < 2 * (S + 1); i += EVENT_THREADS) bins[i] = 0;
    for (int i = tid; i < pitch; i += EVENT_THREADS) {                         // row 0 and column 0 (rows == pitch)
        Tn[i] = 0;
        To[i] = 0;
        Tn[i * pitch] = 0;
        To[i * pitch] = 0;
    }
    __syncthreads();
    for (int i = tid; i < RW * RW; i += EVENT_THREADS) {
        const int ry = i / RW, rx = i - ry * RW;
        const int gy = ty0 - R + ry, gx = tx0 - R + rx;
        int n = 0, o = 0;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const size_t p = (size_t)gy * W + gx;
            n = cp[p];
            const float y = tp[p * tps];
            o = (gt ? y > th : y < th) ? 1 : 0;
            if (ry >= R && ry < R + EVENT_T && rx >= R && rx < R + EVENT_T) {   // a pixel of the tile itself: this block owns it
                if ((unsigned)n <= (unsigned)S) {                              // (a count outside 0..S never indexes the bins)
                    atomicAdd(&bins[n], 1);
                    if (o) atomicAdd(&bins[S + 1 + n], 1);
                }
                if (flags & 1) {
                    const size_t ps4 = (size_t)B * K * hw;
                    int* sp = tsum + ((size_t)b * K + k) * hw + p;
                    int s0 = 0, s1 = 0, s2 = 0, s3 = 0;
                    if (t_before > 0) {
                        s0 = sp[0];
                        s1 = sp[ps4];
                        s2 = sp[2 * ps4];
                        s3 = sp[3 * ps4];
                    }
                    sp[0] = s0 + n;
                    sp[ps4] = s1 + o;
                    sp[2 * ps4] = s2 + n * n;
                    sp[3 * ps4] = s3 + n * o;
                }
            }
        }
        Tn[(ry + 1) * pitch + rx + 1] = n;
        To[(ry + 1) * pitch + rx + 1] = o;
    }
    __syncthreads();
    {
        int* rc = rcnt + (size_t)b * rcs + (size_t)k * (S + 1);
        int* rh = rhit + (size_t)b * rcs + (size_t)k * (S + 1);
        for (int j = tid; j <= S; j += EVENT_THREADS) {
            const int n0 = bins[j], n1 = bins[S + 1 + j];
            if (n0) atomicAdd(rc + j, n0);
            if (n1) atomicAdd(rh + j, n1);
        }
    }
    for (int j = tid; j < 2 * RW; j += EVENT_THREADS) {                        // rows: lanes on consecutive rows, stride pitch (odd)
        int* row = (j < RW ? Tn : To) + ((j < RW ? j : j - RW) + 1) * pitch;
        int run = 0;
        for (int x = 1; x <= RW; ++x) {
            run += row[x];
            row[x] = run;
        }
    }
    __syncthreads();
    for (int j = tid; j < 2 * RW; j += EVENT_THREADS) {                        // columns: lanes on consecutive columns
        int* col = (j < RW ? Tn : To) + (j < RW ? j : j - RW) + 1;
        int run = 0;
        for (int yy = 1; yy <= RW; ++yy) {
            run += col[yy * pitch];
            col[yy * pitch] = run;
        }
    }
    __syncthreads();
    long long acc[EVENT_MAXNS][3];
#pragma unroll
    for (int s = 0; s < EVENT_MAXNS; ++s) acc[s][0] = acc[s][1] = acc[s][2] = 0;
#pragma unroll
    for (int q = 0; q < EVENT_T * EVENT_T / EVENT_THREADS; ++q) {
        const int i = q * EVENT_THREADS + tid;
        const int ly = i / EVENT_T, lx = i % EVENT_T;
        if (ty0 + ly < H && tx0 + lx < W) {
#pragma unroll
            for (int s = 0; s < EVENT_MAXNS; ++s) {
                if (s < NS) {
                    const int r = a.r[s];
                    const int y0 = (ly + R - r) * pitch, y1 = (ly + R + r + 1) * pitch, x0 = lx + R - r, x1 = lx + R + r + 1;
                    const long long nf = (Tn[y1 + x1] - Tn[y0 + x1]) - (Tn[y1 + x0] - Tn[y0 + x0]);
                    const long long no = (To[y1 + x1] - To[y0 + x1]) - (To[y1 + x0] - To[y0 + x0]);
                    acc[s][0] += nf * nf;
                    acc[s][1] += nf * no;
                    acc[s][2] += no * no;
                }
            }
        }
    }
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int s = 0; s < EVENT_MAXNS; ++s) {
#pragma unroll
        for (int v = 0; v < 3; ++v) {
            long long x = acc[s][v];
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) x += __shfl_down(x, d, 64);
            if (lane == 0) red[wave * 3 * EVENT_MAXNS + s * 3 + v] = x;
        }
    }
    __syncthreads();
    if (tid < 3 * NS) {
        const long long x = red[tid] + red[3 * EVENT_MAXNS + tid] + red[2 * 3 * EVENT_MAXNS + tid] + red[3 * 3 * EVENT_MAXNS + tid];
        if (x) atomicAdd((unsigned long long*)(fss + (size_t)b * fcs + (size_t)k * NS * 3 + tid), (unsigned long long)x);
    }
}

extern "C" int tmg_ens_event_step(const void* cnt, const void* target, const int64_t* t_d, const void* thr, const int64_t* ev,
                                  const int64_t* scales, void* rel_count, void* rel_hit, void* fss_raw, void* tsum, const int64_t* o_d,
                                  const int64_t* dims, hipStream_t st) {
    if (!dims) return -3;
    const int64_t S = dims[0], B = dims[1], H = dims[2], W = dims[3], C = dims[4], K = dims[5], NS = dims[6], t_before = dims[7],
                  flags = dims[8];
    if (C < 2 || C > EVENT_MAXC || t_before < 0 || K < 1 || K > EVENT_MAXK || S < 1 || NS < 1) return -1;
    if (t_d && (t_d[0] < C || t_d[1] < 0 || t_d[1] + C > t_d[0])) return -1;
    EventArgs a;
    if (ev && event_args(ev, K, C, &a)) return -1;
    if (o_d && (o_d[0] < K * (S + 1) || o_d[1] < K * NS * 3)) return -1;
    const int64_t pd[6] = {S, B, H, W, K, NS};
    EventPlan q;
    const int rc = event_plan(pd, scales, &q);                                 // its -1, then its -2
    if (rc) return rc;
    if (!t_d || !ev || !o_d || !scales) return -3;
    const int64_t HW = H * W;
    if (t_d[0] >= (1ll << 31) || B * HW * t_d[0] >= (1ll << 40) || B * K * HW >= (1ll << 38)) return -2;
    if (B * o_d[0] >= (1ll << 40) || B * o_d[1] >= (1ll << 40)) return -2;
    if ((flags & 1) && S * S * (t_before + 1) >= (1ll << 31)) return -2;      // the int32 per-pixel sums
    if (!cnt || !target || !thr || !rel_count || !rel_hit || !fss_raw) return -3;
    if ((flags & 1) && !tsum) return -3;
    for (int i = 0; i < EVENT_MAXNS; ++i) a.r[i] = i < NS ? (int)(scales[i] / 2) : 0;
    const int nrel = (int)(K * (S + 1)), nfss = (int)(K * NS * 3);
    const int nz = nrel > nfss ? nrel : nfss;
    hipLaunchKernelGGL(ens_event_zero_kernel, dim3((unsigned)((nz + 255) / 256), (unsigned)B), dim3(256), 0, st, (int*)rel_count,
                       (int*)rel_hit, (long long*)fss_raw, (long long)o_d[0], (long long)o_d[1], nrel, nfss);
    TMG_CHECK_LAUNCH();
    dim3 grid((unsigned)(q.nty * q.ntx), (unsigned)K, (unsigned)B);
    hipLaunchKernelGGL(ens_event_step_kernel, grid, dim3(EVENT_THREADS), (size_t)q.lds, st, (const int*)cnt,
                       (const float*)target + t_d[1], (int)t_d[0], (const float*)thr, (int*)rel_count, (int*)rel_hit, (long long*)fss_raw,
                       (int*)tsum, (long long)o_d[0], (long long)o_d[1], (int)S, (int)B, (int)H, (int)W, (int)K, (int)NS, (int)q.halo,
                       (int)q.ntx, (int)t_before, (int)flags, a);
    TMG_CHECK_LAUNCH();
    return 0;
}
