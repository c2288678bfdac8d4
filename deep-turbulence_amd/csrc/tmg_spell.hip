// Event durations of sampled roll-outs along the time window (tmg_ops.EnsembleSpells / utils.modelPredSpells): how long a pixel of a
// member, or of the target, stays in an event (a spell) and out of it (a gap).  An event k is (channel, raw threshold thr[b][k],
// direction), strict, as in tmg_event.hip; a value that compares false (NaN, or an infinity on the wrong side) is in no event.
// Definitions, layouts and codes: include/tmglow_hip_spell.h.
//   ens_spell_zero_kernel    zeroes the table, launched by the step call of step 0 with row0 = 0
//   ens_spell_step_kernel    one chunk of k whole rows at window step t: reads the chunk's NHWC rows directly, advances the state word
//                            of every (row, case, event, pixel) and counts the runs that end at this step
//   ens_spell_final_kernel   once: counts the runs that are still open and folds every row's longest spell over the members
// A streaming state machine: one 32-bit word per (row, case, event, pixel) in the planar buffer state [S + 1][B][K][HW] is read,
// advanced and written back once per step (step 0 writes without reading).  One thread owns one pixel of one case and loops over the
// chunk's rows; state and maps are planar, lanes on consecutive pixels: their traffic is coalesced, and every word has one writer.
// Ended runs are counted into a per-block LDS table of one group of G rows (int32 LDS atomics; a block holds 256 pixels and a run is
// at most 32767 long: the sums stay under 2^23), and each group is flushed with one 64-bit integer global atomic per non-empty entry.
// Integer adds only: no float arithmetic, no float atomics, so the sums do not depend on the order and every output is bitwise
// reproducible.  Lanes past HW touch no memory and stay for every barrier.  The per-event registers (th, cin, csp, ...) are indexed by
// compile-time constants in unrolled loops: no scratch.
#include "tmg_common.h"
#include "tmglow_hip_spell.h"

#define SPELL_MAXC 4
#define SPELL_MAXK 4
#define SPELL_MAXL 64
#define SPELL_MAXS 1024
#define SPELL_MAXT 32767
#define SPELL_MAXG 8
#define SPELL_LDS 16384
#define SPELL_THREADS 256

struct SpellArgs {
    int ech[SPELL_MAXK];     // the events' channels
    int egt[SPELL_MAXK];     // 1: x > thr, 0: x < thr
};

struct SpellPlan {
    long long blocks, threads, group, lds, state_words, gx, gy, row_words, table_words, fin_lds;
};

// dims = {S, B, HW, K, L, Tn}; -> 0 and the plan, or the code
static int spell_plan(const int64_t* dims, SpellPlan* q) {
    const int64_t S = dims[0], B = dims[1], HW = dims[2], K = dims[3], L = dims[4], Tn = dims[5];
    if (S < 1 || B < 1 || HW < 1 || K < 1 || K > SPELL_MAXK || L < 1 || L > SPELL_MAXL || Tn < 2) return -1;
    if (S > SPELL_MAXS || B > 65535 || Tn > SPELL_MAXT || S * Tn >= (1ll << 31) || HW >= (1ll << 31) - 256) return -2;
    if ((S + 1) * B * K * HW >= (1ll << 40)) return -2;
    const int64_t per = 4 * K * 2 * (L + 3);                                   // the LDS bytes of one row of the group
    int64_t G = SPELL_LDS / per;
    G = G > SPELL_MAXG ? SPELL_MAXG : G;
    q->group = G;
    q->lds = G * per;
    q->fin_lds = G * K * 2 * 4 * 4;
    q->threads = SPELL_THREADS;
    q->gx = (HW + SPELL_THREADS - 1) / SPELL_THREADS;
    q->gy = B;
    q->blocks = q->gx * q->gy;
    q->state_words = (S + 1) * B * K * HW;
    q->row_words = L + 7;
    q->table_words = B * K * (S + 1) * 2 * q->row_words;
    return 0;
}

extern "C" int tmg_ens_spell_plan(const int64_t* dims, int64_t* out) {
    if (!dims) return -3;
    SpellPlan q;
    const int rc = spell_plan(dims, &q);
    if (rc) return rc;
    if (!out) return -3;
    const long long v[10] = {q.blocks, q.threads, q.group, q.lds, q.state_words, q.gx, q.gy, q.row_words, q.table_words, q.fin_lds};
    for (int i = 0; i < 10; ++i) out[i] = v[i];
    return 0;
}

__global__ __launch_bounds__(256) void ens_spell_zero_kernel(unsigned long long* __restrict__ table, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) table[i] = 0ull;
}

// The state word: length | polarity << 15 | longest << 16 | contains-step-0 << 31.
__device__ __forceinline__ unsigned spell_pack(int len, int pol, int lng, int f0) {
    return (unsigned)len | ((unsigned)pol << 15) | ((unsigned)lng << 16) | ((unsigned)f0 << 31);
}

__global__ __launch_bounds__(SPELL_THREADS) void ens_spell_step_kernel(const float* __restrict__ y, int ps, const float* __restrict__ thr,
                                                                       unsigned* __restrict__ state, unsigned long long* __restrict__ table,
                                                                       int* __restrict__ maps, int B, int HW, int K, int L, int S, int k,
                                                                       int row0, int t, int G, SpellArgs a) {
    extern __shared__ int lds[];
    const int tid = threadIdx.x;
    const int p = blockIdx.x * SPELL_THREADS + tid;
    const int b = blockIdx.y;
    const bool active = p < HW;                                               // a lane past the field stays for the barriers
    const size_t hw = (size_t)HW;
    const int EW = L + 3;                                                      // LDS words per (row, event, polarity)
    const int RW = L + 7;                                                      // table words per (case, event, row, polarity)
    float th[SPELL_MAXK];
    int cin[SPELL_MAXK], csp[SPELL_MAXK];
#pragma unroll
    for (int e = 0; e < SPELL_MAXK; ++e) {
        th[e] = e < K ? thr[(size_t)b * K + e] : 0.f;
        cin[e] = 0;
        csp[e] = 0;
    }
    const int nmax = G * K * 2 * EW;
    for (int i = tid; i < nmax; i += SPELL_THREADS) lds[i] = 0;
    __syncthreads();
    for (int g0 = 0; g0 < k; g0 += G) {
        const int gn = k - g0 < G ? k - g0 : G;
        if (active) {
            for (int jj = 0; jj < gn; ++jj) {
                const int j = g0 + jj;
                const float* yp = y + ((size_t)(j * B + b) * hw + p) * ps;
#pragma unroll
                for (int e = 0; e < SPELL_MAXK; ++e) {
                    if (e < K) {
                        const float v = yp[a.ech[e]];
                        const int in = (a.egt[e] ? v > th[e] : v < th[e]) ? 1 : 0;
                        unsigned* sp = state + (((size_t)(row0 + j) * B + b) * K + e) * hw + p;
                        unsigned w;
                        if (t == 0) {
                            w = spell_pack(1, in, in, 1);
                            csp[e] += in;
                        } else {
                            const unsigned w0 = *sp;
                            int len = (int)(w0 & 0x7fffu), pol = (int)((w0 >> 15) & 1u), lng = (int)((w0 >> 16) & 0x7fffu);
                            int f0 = (int)(w0 >> 31);
                            if (in == pol) {
                                len += 1;
                            } else {                                           // the run ends: left when it held step 0, else complete
                                int* q = lds + ((jj * K + e) * 2 + pol) * EW;
                                if (f0) {
                                    atomicAdd(q + L + 1, 1);
                                    atomicAdd(q + L + 2, len);
                                } else {
                                    const int bin = (len < L ? len : L) - 1;    // (len >= 1 once step 0 has written the word)
                                    atomicAdd(q + (bin > 0 ? bin : 0), 1);
                                    atomicAdd(q + L, len);
                                }
                                len = 1;
                                pol = in;
                                f0 = 0;
                                csp[e] += in;
                            }
                            if (pol && len > lng) lng = len;
                            w = spell_pack(len, pol, lng, f0);
                        }
                        *sp = w;
                        cin[e] += in;
                    }
                }
            }
        }
        __syncthreads();
        const int n = gn * K * 2 * EW;
        for (int i = tid; i < n; i += SPELL_THREADS) {                         // flush the group and leave the table zero
            const int v = lds[i];
            if (v) {
                lds[i] = 0;
                const int wd = i % EW;
                int r = i / EW;
                const int pol = r & 1;
                r >>= 1;
                const int e = r % K, jj = r / K;
                const int dst = wd <= L ? wd : (wd == L + 1 ? L + 1 : L + 4);
                unsigned long long* tp = table + ((((size_t)b * K + e) * (S + 1) + (row0 + g0 + jj)) * 2 + pol) * RW + dst;
                atomicAdd(tp, (unsigned long long)v);
            }
        }
        __syncthreads();
    }
    if (active) {
        const size_t plane = (size_t)B * K * hw;
        int* mp = maps + (row0 == S ? 4 * plane : 0);
        const bool first = t == 0 && (row0 == 0 || row0 == S);                 // the plane's first writer: written, not read
#pragma unroll
        for (int e = 0; e < SPELL_MAXK; ++e) {
            if (e < K) {
                int* m = mp + ((size_t)b * K + e) * hw + p;
                m[0] = (first ? 0 : m[0]) + cin[e];
                m[plane] = (first ? 0 : m[plane]) + csp[e];
            }
        }
    }
}

__global__ __launch_bounds__(SPELL_THREADS) void ens_spell_final_kernel(const unsigned* __restrict__ state,
                                                                        unsigned long long* __restrict__ table, int* __restrict__ maps,
                                                                        int B, int HW, int K, int L, int S, int G) {
    extern __shared__ int lds[];
    const int tid = threadIdx.x;
    const int p = blockIdx.x * SPELL_THREADS + tid;
    const int b = blockIdx.y;
    const bool active = p < HW;
    const size_t hw = (size_t)HW;
    const int RW = L + 7;
    int lsum[SPELL_MAXK], lmax[SPELL_MAXK], ltgt[SPELL_MAXK];
#pragma unroll
    for (int e = 0; e < SPELL_MAXK; ++e) lsum[e] = lmax[e] = ltgt[e] = 0;
    const int nmax = G * K * 2 * 4;
    for (int i = tid; i < nmax; i += SPELL_THREADS) lds[i] = 0;
    __syncthreads();
    for (int g0 = 0; g0 <= S; g0 += G) {
        const int gn = S + 1 - g0 < G ? S + 1 - g0 : G;
        if (active) {
            for (int jj = 0; jj < gn; ++jj) {
                const int row = g0 + jj;
#pragma unroll
                for (int e = 0; e < SPELL_MAXK; ++e) {
                    if (e < K) {
                        const unsigned w0 = state[(((size_t)row * B + b) * K + e) * hw + p];
                        const int len = (int)(w0 & 0x7fffu), pol = (int)((w0 >> 15) & 1u), lng = (int)((w0 >> 16) & 0x7fffu);
                        const int f0 = (int)(w0 >> 31);
                        int* q = lds + ((jj * K + e) * 2 + pol) * 4 + (f0 ? 2 : 0);    // right, or both when it held step 0
                        atomicAdd(q, 1);
                        atomicAdd(q + 1, len);
                        if (row < S) {
                            lsum[e] += lng;
                            lmax[e] = lng > lmax[e] ? lng : lmax[e];
                        } else {
                            ltgt[e] = lng;
                        }
                    }
                }
            }
        }
        __syncthreads();
        const int n = gn * K * 2 * 4;
        for (int i = tid; i < n; i += SPELL_THREADS) {
            const int v = lds[i];
            if (v) {
                lds[i] = 0;
                const int wd = i & 3;
                int r = i >> 2;
                const int pol = r & 1;
                r >>= 1;
                const int e = r % K, jj = r / K;
                const int dst = wd == 0 ? L + 2 : (wd == 1 ? L + 5 : (wd == 2 ? L + 3 : L + 6));
                unsigned long long* tp = table + ((((size_t)b * K + e) * (S + 1) + (g0 + jj)) * 2 + pol) * RW + dst;
                atomicAdd(tp, (unsigned long long)v);
            }
        }
        __syncthreads();
    }
    if (active) {
        const size_t plane = (size_t)B * K * hw;
#pragma unroll
        for (int e = 0; e < SPELL_MAXK; ++e) {
            if (e < K) {
                int* m = maps + ((size_t)b * K + e) * hw + p;
                m[2 * plane] = lsum[e];
                m[3 * plane] = lmax[e];
                m[6 * plane] = ltgt[e];
            }
        }
    }
}

// ev: K x (channel, direction) host integers -> the kernel's argument block, or -1
static int spell_args(const int64_t* ev, int64_t K, int64_t C, SpellArgs* a) {
    for (int e = 0; e < SPELL_MAXK; ++e) {
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

extern "C" int tmg_ens_spell_step(const void* y, const int64_t* y_d, const void* thr, const int64_t* ev, void* state, void* table,
                                  void* maps, const int64_t* dims, hipStream_t st) {
    if (!dims) return -3;
    const int64_t k = dims[0], B = dims[1], HW = dims[2], C = dims[3], S = dims[4], row0 = dims[5], K = dims[6], L = dims[7], Tn = dims[8],
                  t = dims[9];
    if (C < 2 || C > SPELL_MAXC || k < 1 || row0 < 0 || t < 0 || t >= Tn || K < 1 || K > SPELL_MAXK) return -1;
    if (!(row0 + k <= S || (row0 == S && k == 1))) return -1;
    if (y_d && (y_d[0] < C || y_d[1] < 0 || y_d[1] + C > y_d[0])) return -1;
    SpellArgs a;
    if (ev && spell_args(ev, K, C, &a)) return -1;
    const int64_t pd[6] = {S, B, HW, K, L, Tn};
    SpellPlan q;
    const int rc = spell_plan(pd, &q);                                         // its -1, then its -2
    if (rc) return rc;
    if (!y_d || !ev) return -3;
    if (y_d[0] >= (1ll << 31) || (k * B) * HW * y_d[0] >= (1ll << 40)) return -2;
    if (!y || !thr || !state || !table || !maps) return -3;
    if (t == 0 && row0 == 0) {
        hipLaunchKernelGGL(ens_spell_zero_kernel, dim3((unsigned)((q.table_words + 255) / 256)), dim3(256), 0, st,
                           (unsigned long long*)table, (long long)q.table_words);
        TMG_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(ens_spell_step_kernel, dim3((unsigned)q.gx, (unsigned)q.gy), dim3(SPELL_THREADS), (size_t)q.lds, st,
                       (const float*)y + y_d[1], (int)y_d[0], (const float*)thr, (unsigned*)state, (unsigned long long*)table, (int*)maps,
                       (int)B, (int)HW, (int)K, (int)L, (int)S, (int)k, (int)row0, (int)t, (int)q.group, a);
    TMG_CHECK_LAUNCH();
    return 0;
}

extern "C" int tmg_ens_spell_finalize(const void* state, void* table, void* maps, const int64_t* dims, hipStream_t st) {
    if (!dims) return -3;
    SpellPlan q;
    const int rc = spell_plan(dims, &q);
    if (rc) return rc;
    if (!state || !table || !maps) return -3;
    const int64_t S = dims[0], B = dims[1], HW = dims[2], K = dims[3], L = dims[4];
    hipLaunchKernelGGL(ens_spell_final_kernel, dim3((unsigned)q.gx, (unsigned)q.gy), dim3(SPELL_THREADS), (size_t)q.fin_lds, st,
                       (const unsigned*)state, (unsigned long long*)table, (int*)maps, (int)B, (int)HW, (int)K, (int)L, (int)S,
                       (int)q.group);
    TMG_CHECK_LAUNCH();
    return 0;
}
