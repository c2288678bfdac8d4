// Vortex census of sampled roll-outs and of the target (tmg_ops.EnsembleVortices / utils.modelPredVortices): the Okubo-Weiss class of
// every pixel, the 4-connected components of each class, their int64 measures and a table of them per row, case and timed step.  The
// definitions are stated once in include/tmglow_hip_vortex.h; every fp32 operation of the classification is rounded on its own.
//   ens_vortex_classify_kernel  one thread per pixel of one plane (row, case): the 3x3 stencils of tmg_field.h from global memory
//                               (tmg_ensemble.hip explains why an LDS tile does not pay for NHWC input with a run-time stride), omega,
//                               class, and one integer atomicAdd per wave that holds a rejected pixel.
//   ens_vortex_tile_kernel      one block per 32 x 32 tile of one plane: a union-find over the tile in LDS.  parent[x] <= x always, so
//                               the forest has no cycles and a root is the smallest index of its tree; a link is one LDS atomicMin of
//                               the larger root onto the smaller, retried from the value it displaced when the larger one had stopped
//                               being a root.  The tile's labels leave as global pixel indices (row-major in the tile and in the
//                               field: the smallest local index is the smallest global one).
//   ens_vortex_merge_kernel     one thread per pixel pair across a tile border: the same union on the label plane itself, whose
//                               every access is an agent-scope atomic (a plain load may be served by a stale L1 line or by another
//                               XCD's view).  No block waits for another: a link that loses a race is retried by its own thread from
//                               what it read, and the launch ends when every pair has been united.
//   ens_vortex_root_kernel      one thread per pixel: label = the root of its tree.  Concurrent replacement is benign (a pixel's
//                               label is always an ancestor of it); the accesses stay atomic so that no stale value is walked.
// Every loop above runs at most H W + 1 trips (an index only ever decreases); one that reaches the bound falls out and stores a code
// into the status word with an ordinary store: a wrong kernel ends with a wrong answer, never with a hang.
//   ens_vortex_area_kernel      area[root] += 1 per labelled pixel (int32 atomicAdd).
//   ens_vortex_rank_kernel      one block of 1024 threads per plane: thread t owns a contiguous run of pixels, counts its qualifying
//                               roots, a Hillis-Steele scan over the 1024 counts gives every root its slot = its rank in root order.
//   ens_vortex_fill_kernel      one block per 1024 pixels of one plane: the measures of its pixels into an LDS copy of the table
//                               (64-bit LDS integer atomics), then one global 64-bit atomicAdd / atomicMax per non-zero word.
// Integer sums and maxima do not depend on the order: every output is bitwise reproducible and independent of the chunking.
#include "tmg_field.h"
#include "tmglow_hip.h"
#include "tmglow_hip_vortex.h"

#define VX_TH 32
#define VX_TW 32
#define VX_THREADS 256
#define VX_PPT 4             // pixels per thread of the tile and the fill kernels: 1024 pixels per block
#define VX_RANK_THREADS 1024
#define VX_MAXK 256
#define VX_MAXS 1024
#define VX_MAXSIDE 512
#define VX_WORDS 8

struct VxPlan {
    int64_t nth, ntw, tiles, pairs, merge_blocks, pixel_blocks, lds_label, lds_census, ws, state;
};

static void vx_geometry(int64_t H, int64_t W, VxPlan* q) {
    q->nth = (H + VX_TH - 1) / VX_TH;
    q->ntw = (W + VX_TW - 1) / VX_TW;
    q->tiles = q->nth * q->ntw;
    q->pairs = (q->ntw - 1) * H + (q->nth - 1) * W;
    q->merge_blocks = (q->pairs + VX_THREADS - 1) / VX_THREADS;
    q->pixel_blocks = (H * W + VX_THREADS - 1) / VX_THREADS;
    q->lds_label = 5 * VX_TH * VX_TW;
}

// dims = {k, S, B, H, W, K, Tn}
static int vx_plan(const int64_t* dims, VxPlan* q) {
    const int64_t k = dims[0], S = dims[1], B = dims[2], H = dims[3], W = dims[4], K = dims[5], Tn = dims[6];
    if (k < 1 || S < 1 || B < 1 || H < 3 || W < 3 || K < 1 || K > VX_MAXK || Tn < 1 || k > S + 1) return -1;
    if (S > VX_MAXS || H > VX_MAXSIDE || W > VX_MAXSIDE || k * B > 65535) return -2;
    vx_geometry(H, W, q);
    const int64_t scan = 4 * VX_RANK_THREADS + 16;
    q->lds_census = 64 * K > scan ? 64 * K : scan;
    q->ws = 17 * k * B * H * W;
    q->state = 64 * K * (S + 1) * B * Tn + 16 * B * H * W;
    return 0;
}

extern "C" int tmg_ens_vortex_plan(const int64_t* dims, int64_t* plan) {
    if (!dims) return -3;
    VxPlan q;
    const int rc = vx_plan(dims, &q);
    if (rc) return rc;
    if (!plan) return -3;
    const int64_t v[12] = {VX_TH, VX_TW, q.nth, q.ntw, q.tiles, q.merge_blocks, q.pixel_blocks, VX_THREADS, q.lds_label, q.lds_census,
                           q.ws, q.state};
    for (int i = 0; i < 12; ++i) plan[i] = v[i];
    return 0;
}

// ---- classification -------------------------------------------------------------------------------------------------------------------
#pragma clang fp contract(off)

__global__ __launch_bounds__(VX_THREADS) void ens_vortex_classify_kernel(
    const float* __restrict__ y, int ps, const float* __restrict__ u, const float* __restrict__ out_mu, const float* __restrict__ out_std,
    const float* __restrict__ thr, const float* __restrict__ qscale, float* __restrict__ omega, signed char* __restrict__ cls,
    int* __restrict__ rejected, int B, int Hh, int Ww, int C, float rdx, float rdy) {
    const int row = blockIdx.y;
    const int b = row % B;
    const int HW = Hh * Ww;
    const int p = blockIdx.x * VX_THREADS + threadIdx.x;
    bool rej = false;
    if (p < HW) {
        const float sc0 = u ? u[b * C] : 1.f, sc1 = u ? u[b * C + 1] : 1.f;
        const float mu0 = out_mu[0], mu1 = out_mu[1], sd0 = out_std[0], sd1 = out_std[1];
        const int h = p / Ww, w = p - h * Ww;
        const long long rs = (long long)Ww * ps;
        const float* yp = y + ((size_t)row * HW + p) * ps;
        const bool up = h > 0, dn = h + 1 < Hh, lf = w > 0, rt = w + 1 < Ww;
        const float sxv = tmg_sx<false>(yp, ps, rs, 1, sc1, sd1, mu1, up, dn, lf, rt);
        const float syu = tmg_sy<false>(yp, ps, rs, 0, sc0, sd0, mu0, up, dn, lf, rt);
        const float sxu = tmg_sx<false>(yp, ps, rs, 0, sc0, sd0, mu0, up, dn, lf, rt);
        const float syv = tmg_sy<false>(yp, ps, rs, 1, sc1, sd1, mu1, up, dn, lf, rt);
        const float vx = sxv * rdx, uy = syu * rdy, ux = sxu * rdx, vy = syv * rdy;
        const float om = vx - uy;
        const float sn = ux - vy;
        const float ss = vx + uy;
        const float ww = om * om, nn = sn * sn, s2 = ss * ss;
        float ow = ww - nn;
        ow = ow - s2;
        const float qf = om * qscale[b];
        const bool interior = up && dn && lf && rt;
        const bool over = ow > thr[b];
        const bool fits = fabsf(qf) <= 2147483648.f;
        int c = 0;
        if (interior && over && fits) {
            const long long q = (long long)rintf(qf);
            if (q != 0) c = q > 0 ? 1 : -1;
        }
        rej = interior && (ow != ow || (over && !fits));
        omega[(size_t)row * HW + p] = om;
        cls[(size_t)row * HW + p] = (signed char)c;
    }
    const unsigned long long m = __ballot(rej);
    if (m && (threadIdx.x & 63) == 0) atomicAdd(rejected + row, (int)__popcll(m));
}

extern "C" int tmg_ens_vortex_classify(const void* rows, const int64_t* t_d, const void* u, const void* mu, const void* sd, const void* thr,
                                       const void* qscale, void* omega, void* cls, void* rejected, const float* fl, const int64_t* dims,
                                       hipStream_t st) {
    if (!dims) return -3;
    const int64_t k = dims[0], B = dims[1], H = dims[2], W = dims[3], C = dims[4];
    if (k < 1 || B < 1 || H < 3 || W < 3 || C < 2 || C > 4) return -1;
    if (t_d && (t_d[1] < 0 || t_d[0] < t_d[1] + C)) return -1;
    if (fl && (!(fl[0] > 0.f) || !(fl[1] > 0.f) || !(fl[0] <= 3.0e38f) || !(fl[1] <= 3.0e38f))) return -1;
    if (H > VX_MAXSIDE || W > VX_MAXSIDE || k * B > 65535) return -2;
    if (t_d && t_d[0] >= (1ll << 31)) return -2;
    if (!t_d || !fl || !rows || !mu || !sd || !thr || !qscale || !omega || !cls || !rejected) return -3;
    VxPlan q;
    vx_geometry(H, W, &q);
    hipError_t e = hipMemsetAsync(rejected, 0, (size_t)(k * B) * sizeof(int), st);
    if (e != hipSuccess) return (int)e;
    const float rdx = 0.125f / fl[0], rdy = 0.125f / fl[1];
    hipLaunchKernelGGL(ens_vortex_classify_kernel, dim3((unsigned)q.pixel_blocks, (unsigned)(k * B)), dim3(VX_THREADS), 0, st,
                       (const float*)rows + t_d[1], (int)t_d[0], (const float*)u, (const float*)mu, (const float*)sd, (const float*)thr,
                       (const float*)qscale, (float*)omega, (signed char*)cls, (int*)rejected, (int)B, (int)H, (int)W, (int)C, rdx, rdy);
    TMG_CHECK_LAUNCH();
    return 0;
}

// ---- labelling ------------------------------------------------------------------------------------------------------------------------
// The union-find, once for the tile in LDS (workgroup scope) and once for the label plane (agent scope).  `bound` trips at most.
template <int SCOPE>
__device__ __forceinline__ int vx_find(int* par, int x, int bound, int code, int* __restrict__ status) {
    for (int it = 0; it < bound; ++it) {
        const int p = __hip_atomic_load(par + x, __ATOMIC_RELAXED, SCOPE);
        if (p == x || p < 0) return x;                                         // (p < 0 cannot happen on a labelled pixel)
        x = p;
    }
    *status = code;
    return x;
}

template <int SCOPE>
__device__ __forceinline__ void vx_union(int* par, int a, int b, int bound, int code, int* __restrict__ status) {
    for (int it = 0; it < bound; ++it) {
        a = vx_find<SCOPE>(par, a, bound, code - 1, status);
        b = vx_find<SCOPE>(par, b, bound, code - 1, status);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = __hip_atomic_fetch_min(par + a, b, __ATOMIC_RELAXED, SCOPE);
        if (old == a) return;                                                  // a was a root and now hangs under b
        a = old;                                                               // a had been linked already: unite what it hung under
    }
    *status = code;
}

__global__ __launch_bounds__(VX_THREADS) void ens_vortex_tile_kernel(const signed char* __restrict__ cls, int* __restrict__ label,
                                                                     int* __restrict__ status, int Hh, int Ww, int ntw) {
    __shared__ int par[VX_TH * VX_TW];
    __shared__ signed char lc[VX_TH * VX_TW];
    const int tid = threadIdx.x;
    const int th = blockIdx.x / ntw, tw = blockIdx.x - th * ntw;
    const int h0 = th * VX_TH, w0 = tw * VX_TW;
    const size_t base = (size_t)blockIdx.y * Hh * Ww;
    const int bound = VX_TH * VX_TW + 1;
    for (int q = 0; q < VX_PPT; ++q) {
        const int i = q * VX_THREADS + tid;
        const int h = h0 + i / VX_TW, w = w0 + i % VX_TW;
        lc[i] = (h < Hh && w < Ww) ? cls[base + (size_t)h * Ww + w] : (signed char)0;
        par[i] = i;
    }
    __syncthreads();
    for (int q = 0; q < VX_PPT; ++q) {
        const int i = q * VX_THREADS + tid;
        const signed char c = lc[i];
        if (c) {
            if (i % VX_TW && lc[i - 1] == c) vx_union<__HIP_MEMORY_SCOPE_WORKGROUP>(par, i, i - 1, bound, 2, status);
            if (i >= VX_TW && lc[i - VX_TW] == c) vx_union<__HIP_MEMORY_SCOPE_WORKGROUP>(par, i, i - VX_TW, bound, 2, status);
        }
    }
    __syncthreads();
    for (int q = 0; q < VX_PPT; ++q) {
        const int i = q * VX_THREADS + tid;
        const int h = h0 + i / VX_TW, w = w0 + i % VX_TW;
        if (h < Hh && w < Ww) {
            int g = -1;
            if (lc[i]) {
                const int r = vx_find<__HIP_MEMORY_SCOPE_WORKGROUP>(par, i, bound, 1, status);
                g = (h0 + r / VX_TW) * Ww + w0 + r % VX_TW;
            }
            label[base + (size_t)h * Ww + w] = g;
        }
    }
}

__global__ __launch_bounds__(VX_THREADS) void ens_vortex_merge_kernel(const signed char* __restrict__ cls, int* label,
                                                                      int* __restrict__ status, int Hh, int Ww, int ntw, int pairs) {
    const int i = blockIdx.x * VX_THREADS + threadIdx.x;
    if (i >= pairs) return;
    const size_t base = (size_t)blockIdx.y * Hh * Ww;
    const int nv = (ntw - 1) * Hh;                                             // pairs across the vertical borders come first
    int pa, pb;
    if (i < nv) {
        const int j = i / Hh, h = i - j * Hh;
        pb = h * Ww + (j + 1) * VX_TW;
        pa = pb - 1;
    } else {
        const int r = i - nv;
        const int t = r / Ww, w = r - t * Ww;
        pb = (t + 1) * VX_TH * Ww + w;
        pa = pb - Ww;
    }
    const signed char c = cls[base + pa];
    if (c && cls[base + pb] == c) vx_union<__HIP_MEMORY_SCOPE_AGENT>(label + base, pb, pa, Hh * Ww + 1, 4, status);
}

__global__ __launch_bounds__(VX_THREADS) void ens_vortex_root_kernel(int* label, int* __restrict__ status, int HW) {
    const int p = blockIdx.x * VX_THREADS + threadIdx.x;
    if (p >= HW) return;
    int* lab = label + (size_t)blockIdx.y * HW;
    const int l = __hip_atomic_load(lab + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (l < 0 || l == p) return;
    const int r = vx_find<__HIP_MEMORY_SCOPE_AGENT>(lab, l, HW + 1, 5, status);
    __hip_atomic_store(lab + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

extern "C" int tmg_ens_vortex_label(const void* cls, void* label, void* status, const int64_t* dims, hipStream_t st) {
    if (!dims) return -3;
    const int64_t n = dims[0], H = dims[1], W = dims[2];
    if (n < 1 || H < 1 || W < 1) return -1;
    if (n > 65535 || H > VX_MAXSIDE || W > VX_MAXSIDE) return -2;
    if (!cls || !label || !status) return -3;
    VxPlan q;
    vx_geometry(H, W, &q);
    hipLaunchKernelGGL(ens_vortex_tile_kernel, dim3((unsigned)q.tiles, (unsigned)n), dim3(VX_THREADS), 0, st, (const signed char*)cls,
                       (int*)label, (int*)status, (int)H, (int)W, (int)q.ntw);
    TMG_CHECK_LAUNCH();
    if (q.pairs > 0) {
        hipLaunchKernelGGL(ens_vortex_merge_kernel, dim3((unsigned)q.merge_blocks, (unsigned)n), dim3(VX_THREADS), 0, st,
                           (const signed char*)cls, (int*)label, (int*)status, (int)H, (int)W, (int)q.ntw, (int)q.pairs);
        TMG_CHECK_LAUNCH();
        hipLaunchKernelGGL(ens_vortex_root_kernel, dim3((unsigned)q.pixel_blocks, (unsigned)n), dim3(VX_THREADS), 0, st, (int*)label,
                           (int*)status, (int)(H * W));
        TMG_CHECK_LAUNCH();
    }
    return 0;
}

// ---- census ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VX_THREADS) void ens_vortex_area_kernel(const int* __restrict__ label, int* __restrict__ area, int HW) {
    const int p = blockIdx.x * VX_THREADS + threadIdx.x;
    if (p >= HW) return;
    const size_t base = (size_t)blockIdx.y * HW;
    const int l = label[base + p];
    if (l >= 0 && l < HW) atomicAdd(area + base + l, 1);
}

__global__ __launch_bounds__(VX_RANK_THREADS) void ens_vortex_rank_kernel(
    const int* __restrict__ label, const signed char* __restrict__ cls, const int* __restrict__ area, int* __restrict__ slot,
    long long* __restrict__ table, int* __restrict__ found, int HW, int K, int min_area) {
    __shared__ int cnt[VX_RANK_THREADS];
    __shared__ int fnd[2];
    const int tid = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * HW;
    const int per = (HW + VX_RANK_THREADS - 1) / VX_RANK_THREADS;
    const int p0 = min(tid * per, HW), p1 = min(p0 + per, HW);
    if (tid < 2) fnd[tid] = 0;
    int c = 0, cp = 0;
    for (int p = p0; p < p1; ++p) {
        const bool ok = label[base + p] == p && area[base + p] >= min_area;
        c += ok;
        cp += ok && cls[base + p] > 0;
    }
    cnt[tid] = c;
    __syncthreads();
    if (cp) atomicAdd(&fnd[0], cp);
    if (c - cp) atomicAdd(&fnd[1], c - cp);
    for (int d = 1; d < VX_RANK_THREADS; d <<= 1) {                            // inclusive Hillis-Steele scan
        const int v = tid >= d ? cnt[tid - d] : 0;
        __syncthreads();
        cnt[tid] += v;
        __syncthreads();
    }
    int rank = cnt[tid] - c;
    const int total = cnt[VX_RANK_THREADS - 1];
    long long* tab = table + (size_t)blockIdx.x * K * VX_WORDS;
    for (int p = p0; p < p1; ++p) {
        const bool ok = label[base + p] == p && area[base + p] >= min_area;
        slot[base + p] = ok ? rank : -1;
        if (ok) {
            if (rank < K) {
                tab[rank * VX_WORDS] = p;
                for (int j = 1; j < VX_WORDS; ++j) tab[rank * VX_WORDS + j] = 0;
            }
            ++rank;
        }
    }
    for (int s = total + tid; s < K; s += VX_RANK_THREADS) {
        tab[s * VX_WORDS] = -1;
        for (int j = 1; j < VX_WORDS; ++j) tab[s * VX_WORDS + j] = 0;
    }
    if (tid < 2) found[blockIdx.x * 2 + tid] = fnd[tid];
}

__global__ __launch_bounds__(VX_THREADS) void ens_vortex_fill_kernel(
    const int* __restrict__ label, const signed char* __restrict__ cls, const float* __restrict__ omega, const float* __restrict__ qscale,
    const int* __restrict__ slot, long long* __restrict__ table, int* __restrict__ core, int B, int HW, int Ww, int K) {
    extern __shared__ unsigned long long lt[];                                 // [K][8]
    const int tid = threadIdx.x;
    const int row = blockIdx.y, b = row % B;
    const size_t base = (size_t)row * HW;
    for (int i = tid; i < K * VX_WORDS; i += VX_THREADS) lt[i] = 0ull;
    __syncthreads();
    const float qs = qscale[b];
    for (int j = 0; j < VX_PPT; ++j) {
        const int p = blockIdx.x * VX_THREADS * VX_PPT + j * VX_THREADS + tid;
        if (p >= HW) break;
        const int l = label[base + p];
        if (l < 0 || l >= HW) continue;
        const int s = slot[base + l];
        if (s < 0) continue;
        const int sg = cls[base + p] > 0 ? 0 : 1;
        atomicAdd(core + ((size_t)b * 2 + sg) * HW + p, 1);
        if (s >= K) continue;
        const float qf = omega[base + p] * qs;
        const long long q = (long long)rintf(qf);                              // |qf| <= 2^31 on every classified pixel
        const long long h = p / Ww, w = p - h * Ww;
        unsigned long long* e = lt + s * VX_WORDS;
        atomicAdd(e + 1, 1ull);
        atomicAdd(e + 2, (unsigned long long)w);
        atomicAdd(e + 3, (unsigned long long)h);
        atomicAdd(e + 4, (unsigned long long)q);                               // two's complement: the sum modulo 2^64 is the signed sum
        atomicAdd(e + 5, (unsigned long long)(q * w));
        atomicAdd(e + 6, (unsigned long long)(q * h));
        atomicMax(e + 7, (unsigned long long)(q < 0 ? -q : q));
    }
    __syncthreads();
    unsigned long long* tab = (unsigned long long*)table + (size_t)row * K * VX_WORDS;
    for (int i = tid; i < K * VX_WORDS; i += VX_THREADS) {
        const unsigned long long v = lt[i];
        const int word = i & (VX_WORDS - 1);
        if (word == 0 || v == 0ull) continue;
        if (word == 7)
            atomicMax(tab + i, v);
        else
            atomicAdd(tab + i, v);
    }
}

extern "C" int tmg_ens_vortex_census(const void* label, const void* cls, const void* omega, const void* qscale, void* area, void* slot,
                                     void* table, void* found, void* core, const int64_t* dims, hipStream_t st) {
    if (!dims) return -3;
    const int64_t k = dims[0], B = dims[1], H = dims[2], W = dims[3], K = dims[4], min_area = dims[5];
    if (k < 1 || B < 1 || H < 3 || W < 3 || K < 1 || K > VX_MAXK || min_area < 1) return -1;
    if (H > VX_MAXSIDE || W > VX_MAXSIDE || k * B > 65535 || min_area >= (1ll << 31)) return -2;
    if (!label || !cls || !omega || !qscale || !area || !slot || !table || !found || !core) return -3;
    VxPlan q;
    vx_geometry(H, W, &q);
    const int64_t HW = H * W, n = k * B;
    hipError_t e = hipMemsetAsync(area, 0, (size_t)(n * HW) * sizeof(int), st);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(ens_vortex_area_kernel, dim3((unsigned)q.pixel_blocks, (unsigned)n), dim3(VX_THREADS), 0, st, (const int*)label,
                       (int*)area, (int)HW);
    TMG_CHECK_LAUNCH();
    hipLaunchKernelGGL(ens_vortex_rank_kernel, dim3((unsigned)n), dim3(VX_RANK_THREADS), 0, st, (const int*)label, (const signed char*)cls,
                       (const int*)area, (int*)slot, (long long*)table, (int*)found, (int)HW, (int)K, (int)min_area);
    TMG_CHECK_LAUNCH();
    const unsigned fill_blocks = (unsigned)((HW + VX_THREADS * VX_PPT - 1) / (VX_THREADS * VX_PPT));
    hipLaunchKernelGGL(ens_vortex_fill_kernel, dim3(fill_blocks, (unsigned)n), dim3(VX_THREADS), (size_t)(K * VX_WORDS * 8), st,
                       (const int*)label, (const signed char*)cls, (const float*)omega, (const float*)qscale, (const int*)slot,
                       (long long*)table, (int*)core, (int)B, (int)HW, (int)W, (int)K);
    TMG_CHECK_LAUNCH();
    return 0;
}
