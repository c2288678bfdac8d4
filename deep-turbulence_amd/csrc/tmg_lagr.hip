// Lagrangian transport of sampled roll-outs and of the target (tmg_ops.EnsembleTransport / utils.modelPredTransport): pathlines of a
// lattice of seed particles through every row's own velocity field, the flow map's finite-time Lyapunov exponent, displacements,
// residence times and the endpoints' spread against their error.  Rows are the S members plus the target as row S.  The definitions
// (positions, velocity, bilinear value, time interpolation, the Heun step, seeds, residence) are stated once in
// include/tmglow_hip_lagr.h; every fp32 operation below is rounded on its own (no contraction): a float32 host mirror gives the same
// bits.
//   ens_lagr_advect_kernel    one thread per particle of one row of one case (grid NT x B x k).  The only kernel of the library whose
//                             loads are data-dependent gathers: per Heun substep 2 positions x 2 time levels x 2 components x 4
//                             corners = 32 dword loads, 16 from prev (planes) and 16 from the NHWC rows (the two channels of a pixel
//                             are adjacent dwords).  There is nothing to stage: a particle's stencil is known only after its
//                             previous substep, and neighbouring particles drift apart, so an LDS tile would be filled by the same
//                             gathers.  What helps instead: particle p = i Gw + j, so the 64 lanes of a wave start on one lattice row
//                             and their corners share cache lines for as long as the flow keeps neighbours together; the kernel
//                             holds no arrays and few registers, so that many waves per SIMD hide the latency of the dependent
//                             loads (the k1 gathers, then the k2 gathers, n times); all 16 loads of one velocity are issued
//                             before its arithmetic.  Safety: the inside test comes before any index is formed, every gather index
//                             is clamped as an integer immediately before its load, and a position read from the state is tested
//                             like any other, so that no value, non-finite ones included, addresses anything outside the row's field
//                             or outside prev.  No division, square root or transcendental reaches the state.
//   ens_lagr_store_kernel<V>  one thread per pixel (V = 0) or per four consecutive pixels (V = 1, 16-byte plane stores) of one row
//                             of one case: prev = fl(fl(a y) + o).  Launched AFTER the advection of the same rows on the same
//                             stream: the advection reads the planes this kernel overwrites.
//   ens_lagr_finalize_kernel  once per mini-batch: one thread per (case, lattice node) loops over the S + 1 rows in fp64: FTLE from
//                             central differences of the final positions, displacement, residence time, endpoint error and spread,
//                             Welford mean / M2 over the members valid at the node, in member order.
#include "tmg_common.h"
#include "tmglow_hip.h"
#include "tmglow_hip_lagr.h"

#define LAGR_MAXS 1024
#define LAGR_THREADS 256
#define LAGR_MAXBOX 4
#define LAGR_MAXSUB 8
#define LAGR_OUTS 17

struct LagrPlan {
    int64_t tile, tiles, stile, stiles, vec;
};

// vec_ok: the base of prev is 16-byte aligned.  W % 4 == 0 makes every plane of prev start on a 16-byte boundary.
static LagrPlan lagr_plan(int64_t Hh, int64_t Ww, int64_t P, int vec_ok) {
    LagrPlan g;
    g.tile = LAGR_THREADS;
    g.tiles = (P + g.tile - 1) / g.tile;
    g.vec = (vec_ok && Ww % 4 == 0) ? 1 : 0;
    g.stile = g.vec ? 4 * LAGR_THREADS : LAGR_THREADS;
    g.stiles = (Hh * Ww + g.stile - 1) / g.stile;
    return g;
}

struct LagrSeeds {
    int Gh, Gw, oy, ox, sy, sx, R, n;
    int box[4 * LAGR_MAXBOX];
};

struct LagrSteps {
    float s[LAGR_MAXSUB + 1];
    float h, hh;
};

__device__ __forceinline__ bool lagr_inside(float px, float py, float wm, float hm) {
    return px >= 0.f && px <= wm && py >= 0.f && py <= hm;                      // a NaN fails: outside
}

// The velocity V(s) of one row at an INSIDE position: bilinear in prev (v0) and in the converted current row (v1), then in time.
__device__ __forceinline__ void lagr_velocity(const float* __restrict__ yp, int ps, const float* __restrict__ pp, float a0, float a1,
                                              float o0, float o1, int Hh, int Ww, float px, float py, float s, float& ku, float& kv) {
#pragma clang fp contract(off)
    int j0 = min((int)floorf(px), Ww - 2), i0 = min((int)floorf(py), Hh - 2);
    j0 = max(0, min(j0, Ww - 2));                                              // the clamps: integers, immediately before the loads
    i0 = max(0, min(i0, Hh - 2));
    const float fx = px - (float)j0, fy = py - (float)i0;
    const size_t hw = (size_t)Hh * Ww;
    const size_t q0 = (size_t)i0 * Ww + j0, q1 = q0 + Ww;                      // q1 + 1 <= (H - 1) W + W - 1 = HW - 1
    const float* y00 = yp + q0 * ps;
    const float* y10 = yp + q1 * ps;
    // all 16 loads first
    const float p00u = pp[q0], p01u = pp[q0 + 1], p10u = pp[q1], p11u = pp[q1 + 1];
    const float p00v = pp[hw + q0], p01v = pp[hw + q0 + 1], p10v = pp[hw + q1], p11v = pp[hw + q1 + 1];
    const float r00u = y00[0], r00v = y00[1], r01u = y00[ps], r01v = y00[ps + 1];
    const float r10u = y10[0], r10v = y10[1], r11u = y10[ps], r11v = y10[ps + 1];
    const float c00u = a0 * r00u + o0, c01u = a0 * r01u + o0, c10u = a0 * r10u + o0, c11u = a0 * r11u + o0;
    const float c00v = a1 * r00v + o1, c01v = a1 * r01v + o1, c10v = a1 * r10v + o1, c11v = a1 * r11v + o1;
    const float t0u = p00u + fx * (p01u - p00u), b0u = p10u + fx * (p11u - p10u), v0u = t0u + fy * (b0u - t0u);
    const float t0v = p00v + fx * (p01v - p00v), b0v = p10v + fx * (p11v - p10v), v0v = t0v + fy * (b0v - t0v);
    const float t1u = c00u + fx * (c01u - c00u), b1u = c10u + fx * (c11u - c10u), v1u = t1u + fy * (b1u - t1u);
    const float t1v = c00v + fx * (c01v - c00v), b1v = c10v + fx * (c11v - c10v), v1v = t1v + fy * (b1v - t1v);
    ku = v0u + s * (v1u - v0u);
    kv = v0v + s * (v1v - v0v);
}

__global__ __launch_bounds__(LAGR_THREADS) void ens_lagr_advect_kernel(const float* __restrict__ y, int ps, const float* __restrict__ a,
                                                                       const float* __restrict__ o, const float* __restrict__ prev,
                                                                       float* __restrict__ pos, int* __restrict__ exitp,
                                                                       int* __restrict__ res, LagrSeeds g, LagrSteps hs, int B, int Hh,
                                                                       int Ww, int row0, int adv) {
#pragma clang fp contract(off)
    const int P = g.Gh * g.Gw;
    const int p = blockIdx.x * LAGR_THREADS + threadIdx.x;
    if (p >= P) return;
    const int b = blockIdx.y, s = blockIdx.z, row = row0 + s;
    const size_t rb = (size_t)row * B + b;
    float* xp = pos + rb * 2 * P + p;
    int* ep = exitp + rb * P + p;
    int* rp = res + rb * g.R * P + p;
    const float wm = (float)(Ww - 1), hm = (float)(Hh - 1);
    float px, py;
    if (adv < 0) {                                                             // the first timed step seeds; prev is not read
        const int i = p / g.Gw, j = p - i * g.Gw;
        px = (float)(g.ox + j * g.sx);
        py = (float)(g.oy + i * g.sy);
        xp[0] = px, xp[P] = py;
        *ep = -1;
        for (int r = 0; r < g.R; ++r) {
            const bool in = py >= (float)g.box[4 * r] && py <= (float)g.box[4 * r + 1] && px >= (float)g.box[4 * r + 2] &&
                            px <= (float)g.box[4 * r + 3];
            rp[(size_t)r * P] = in ? 1 : 0;
        }
        return;
    }
    if (*ep >= 0) return;                                                      // dead: never touched again
    px = xp[0], py = xp[P];
    if (!lagr_inside(px, py, wm, hm)) return;                                  // (a state this kernel did not write: nothing is gathered)
    const size_t hw = (size_t)Hh * Ww;
    const float* yp = y + ((size_t)s * B + b) * hw * ps;
    const float* pp = prev + rb * 2 * hw;
    const float a0 = a[b * 2], a1 = a[b * 2 + 1], o0 = o[b * 2], o1 = o[b * 2 + 1];
    bool dead = false;
    for (int j = 0; j < g.n; ++j) {
        float k1u, k1v, k2u, k2v;
        lagr_velocity(yp, ps, pp, a0, a1, o0, o1, Hh, Ww, px, py, hs.s[j], k1u, k1v);
        const float xs = px + hs.h * k1u, ys = py + hs.h * k1v;
        if (!lagr_inside(xs, ys, wm, hm)) {
            dead = true;
            break;
        }
        lagr_velocity(yp, ps, pp, a0, a1, o0, o1, Hh, Ww, xs, ys, hs.s[j + 1], k2u, k2v);
        const float xn = px + hs.hh * (k1u + k2u), yn = py + hs.hh * (k1v + k2v);
        if (!lagr_inside(xn, yn, wm, hm)) {
            dead = true;
            break;
        }
        px = xn, py = yn;
    }
    xp[0] = px, xp[P] = py;                                                    // (dead: the last inside position)
    if (dead) {
        *ep = adv;
        return;
    }
    for (int r = 0; r < g.R; ++r) {
        const bool in = py >= (float)g.box[4 * r] && py <= (float)g.box[4 * r + 1] && px >= (float)g.box[4 * r + 2] &&
                        px <= (float)g.box[4 * r + 3];
        if (in) rp[(size_t)r * P] += 1;
    }
}

template <int V>
__global__ __launch_bounds__(LAGR_THREADS) void ens_lagr_store_kernel(const float* __restrict__ y, int ps, const float* __restrict__ a,
                                                                      const float* __restrict__ o, float* __restrict__ prev, int B, int HW,
                                                                      int row0) {
#pragma clang fp contract(off)
    constexpr int PX = V ? 4 : 1;
    const long long q = ((long long)blockIdx.x * LAGR_THREADS + threadIdx.x) * PX;
    if (q >= HW) return;                                                       // (V: HW % 4 == 0, so q + 3 < HW)
    const int b = blockIdx.y, s = blockIdx.z;
    const size_t hw = (size_t)HW;
    const float a0 = a[b * 2], a1 = a[b * 2 + 1], o0 = o[b * 2], o1 = o[b * 2 + 1];
    const float* yp = y + (((size_t)s * B + b) * hw + (size_t)q) * ps;
    float* pp = prev + ((size_t)(row0 + s) * B + b) * 2 * hw + (size_t)q;
    float cu[PX], cv[PX];
#pragma unroll
    for (int j = 0; j < PX; ++j) {
        const float ru = yp[(size_t)j * ps], rv = yp[(size_t)j * ps + 1];
        cu[j] = a0 * ru + o0;
        cv[j] = a1 * rv + o1;
    }
    if constexpr (V) {
        *reinterpret_cast<float4*>(pp) = make_float4(cu[0], cu[1], cu[2], cu[3]);
        *reinterpret_cast<float4*>(pp + hw) = make_float4(cv[0], cv[1], cv[2], cv[3]);
    } else {
        pp[0] = cu[0];
        pp[hw] = cv[0];
    }
}

struct LagrFl {
    double dx, dy, step_dt, T_int;
};

struct LagrOuts {
    void* p[LAGR_OUTS];
};

struct LagrWelford {
    double mean, m2;
    int n;
};

__device__ __forceinline__ void lagr_push(LagrWelford& w, double v) {
#pragma clang fp contract(off)
    w.n += 1;
    const double d = v - w.mean;
    w.mean = w.mean + d / (double)w.n;
    w.m2 = w.m2 + d * (v - w.mean);
}

__device__ __forceinline__ double lagr_mean(const LagrWelford& w) { return w.n ? w.mean : __builtin_nan(""); }

__device__ __forceinline__ double lagr_var(const LagrWelford& w) {
    return w.n ? (w.m2 < 0.0 ? 0.0 : w.m2) / (double)w.n : __builtin_nan("");
}

__global__ __launch_bounds__(LAGR_THREADS) void ens_lagr_finalize_kernel(const float* __restrict__ pos, const int* __restrict__ exitp,
                                                                         const int* __restrict__ res, LagrFl fl, LagrOuts out,
                                                                         LagrSeeds g, int S, int B) {
#pragma clang fp contract(off)
    const int P = g.Gh * g.Gw;
    const int p = blockIdx.x * LAGR_THREADS + threadIdx.x;
    const int b = blockIdx.y;
    if (p >= P) return;
    const int i = p / g.Gw, j = p - i * g.Gw;
    const bool interior = i > 0 && i + 1 < g.Gh && j > 0 && j + 1 < g.Gw;
    const double nanv = __builtin_nan("");
    const double x0 = (double)(float)(g.ox + j * g.sx), y0 = (double)(float)(g.oy + i * g.sy);
    const double ddx = (2.0 * (double)g.sx) * fl.dx, ddy = (2.0 * (double)g.sy) * fl.dy, t2 = 2.0 * fl.T_int;
    const size_t bp = (size_t)b * P + p;
    // the target's endpoint first: the members' error is taken against it
    const size_t tb = (size_t)S * B + b;
    const bool talive = exitp[tb * P + p] < 0;
    const double XT = (double)pos[tb * 2 * P + p] * fl.dx, YT = (double)pos[tb * 2 * P + P + p] * fl.dy;
    LagrWelford wf = {0.0, 0.0, 0}, wdx = wf, wdy = wf, wex = wf, wey = wf, werr = wf, wres[LAGR_MAXBOX] = {wf, wf, wf, wf};
    for (int r = 0; r <= S; ++r) {
        const size_t rb = (size_t)r * B + b;
        const float* xp = pos + rb * 2 * P + p;
        const int* ep = exitp + rb * P + p;
        const int ex = ep[0];
        const bool alive = ex < 0;
        const double X = (double)xp[0] * fl.dx, Y = (double)xp[P] * fl.dy;
        const bool valid = interior && alive && ep[-1] < 0 && ep[1] < 0 && ep[-g.Gw] < 0 && ep[g.Gw] < 0;
        double ftle = nanv;
        if (valid) {
            const double F11 = ((double)xp[1] * fl.dx - (double)xp[-1] * fl.dx) / ddx;
            const double F21 = ((double)xp[P + 1] * fl.dy - (double)xp[P - 1] * fl.dy) / ddx;
            const double F12 = ((double)xp[g.Gw] * fl.dx - (double)xp[-g.Gw] * fl.dx) / ddy;
            const double F22 = ((double)xp[P + g.Gw] * fl.dy - (double)xp[P - g.Gw] * fl.dy) / ddy;
            const double C11 = F11 * F11 + F21 * F21, C12 = F11 * F12 + F21 * F22, C22 = F12 * F12 + F22 * F22;
            const double hd = 0.5 * (C11 - C22);
            const double lam = 0.5 * (C11 + C22) + sqrt(hd * hd + C12 * C12);
            ftle = log(lam) / t2;
        }
        const double ddX = ((double)xp[0] - x0) * fl.dx, ddY = ((double)xp[P] - y0) * fl.dy;
        if (r < S) {
            if (valid) lagr_push(wf, ftle);
            if (alive) {
                lagr_push(wdx, ddX), lagr_push(wdy, ddY);
                lagr_push(wex, X), lagr_push(wey, Y);
                if (talive) {
                    const double ex_ = X - XT, ey_ = Y - YT;
                    lagr_push(werr, sqrt(ex_ * ex_ + ey_ * ey_));
                }
            }
#pragma unroll
            for (int q = 0; q < LAGR_MAXBOX; ++q)
                if (q < g.R) lagr_push(wres[q], (double)res[(rb * g.R + q) * P + p] * fl.step_dt);
            if (out.p[14]) {
                const size_t mb = ((size_t)b * S + r) * P + p;
                ((float*)out.p[14])[mb] = (float)ftle;
                ((float*)out.p[15])[((size_t)b * S + r) * 2 * P + p] = xp[0];
                ((float*)out.p[15])[((size_t)b * S + r) * 2 * P + P + p] = xp[P];
                ((int*)out.p[16])[mb] = ex;
            }
        } else {
            ((float*)out.p[2])[bp] = (float)ftle;
            ((float*)out.p[6])[(size_t)b * 2 * P + p] = alive ? (float)ddX : (float)nanv;
            ((float*)out.p[6])[(size_t)b * 2 * P + P + p] = alive ? (float)ddY : (float)nanv;
            ((float*)out.p[8])[bp] = alive ? 1.f : 0.f;
            for (int q = 0; q < g.R; ++q)
                ((float*)out.p[11])[((size_t)b * g.R + q) * P + p] = (float)((double)res[(rb * g.R + q) * P + p] * fl.step_dt);
        }
    }
    ((float*)out.p[0])[bp] = (float)lagr_mean(wf);
    ((float*)out.p[1])[bp] = (float)sqrt(lagr_var(wf));
    ((int*)out.p[3])[bp] = wf.n;
    ((float*)out.p[4])[(size_t)b * 2 * P + p] = (float)lagr_mean(wdx);
    ((float*)out.p[4])[(size_t)b * 2 * P + P + p] = (float)lagr_mean(wdy);
    ((float*)out.p[5])[(size_t)b * 2 * P + p] = (float)sqrt(lagr_var(wdx));
    ((float*)out.p[5])[(size_t)b * 2 * P + P + p] = (float)sqrt(lagr_var(wdy));
    ((float*)out.p[7])[bp] = (float)((double)wex.n / (double)S);
#pragma unroll
    for (int q = 0; q < LAGR_MAXBOX; ++q) {
        if (q < g.R) {
            ((float*)out.p[9])[((size_t)b * g.R + q) * P + p] = (float)lagr_mean(wres[q]);
            ((float*)out.p[10])[((size_t)b * g.R + q) * P + p] = (float)sqrt(lagr_var(wres[q]));
        }
    }
    ((float*)out.p[12])[bp] = (float)lagr_mean(werr);
    ((float*)out.p[13])[bp] = (float)sqrt(lagr_var(wex) + lagr_var(wey));
}

static int lagr_sizes(int64_t S, int64_t B, int64_t Hh, int64_t Ww, int64_t P) {
    if (S < 1 || B < 1 || Hh < 2 || Ww < 2 || P < 1) return -1;
    if (S > LAGR_MAXS || B > 65535 || Hh >= (1ll << 31) || Ww >= (1ll << 31) || Hh * Ww >= (1ll << 31) - 4 * LAGR_THREADS ||
        (S + 1) * B * 2 * Hh * Ww >= (1ll << 40))
        return -2;
    if (P > Hh * Ww) return -1;
    return 0;
}

// The lattice and the boxes against the field -> 0 or -1; fills g.
static int lagr_seeds(const int64_t* sd, int64_t Hh, int64_t Ww, LagrSeeds& g) {
    const int64_t Gh = sd[0], Gw = sd[1], oy = sd[2], ox = sd[3], sy = sd[4], sx = sd[5], R = sd[6], n = sd[7];
    if (Gh < 1 || Gw < 1 || oy < 0 || ox < 0 || sy < 1 || sx < 1 || R < 0 || R > LAGR_MAXBOX || n < 1 || n > LAGR_MAXSUB) return -1;
    if (Gh > Hh || Gw > Ww || sy > Hh || sx > Ww || oy + (Gh - 1) * sy > Hh - 1 || ox + (Gw - 1) * sx > Ww - 1) return -1;
    for (int r = 0; r < LAGR_MAXBOX; ++r) {
        const int64_t* bx = sd + 8 + 4 * r;
        if (r < R && (bx[0] < 0 || bx[1] < bx[0] || bx[1] > Hh - 1 || bx[2] < 0 || bx[3] < bx[2] || bx[3] > Ww - 1)) return -1;
        for (int q = 0; q < 4; ++q) g.box[4 * r + q] = r < R ? (int)bx[q] : 0;
    }
    g.Gh = (int)Gh, g.Gw = (int)Gw, g.oy = (int)oy, g.ox = (int)ox, g.sy = (int)sy, g.sx = (int)sx, g.R = (int)R, g.n = (int)n;
    return 0;
}

extern "C" int tmg_ens_lagr_plan(const int64_t* dims, int64_t* plan) {
    if (!dims) return -3;
    const int rc = lagr_sizes(dims[0], dims[1], dims[2], dims[3], dims[4]);
    if (rc != 0) return rc;
    if (!plan) return -3;
    const LagrPlan g = lagr_plan(dims[2], dims[3], dims[4], 1);
    plan[0] = g.tile;
    plan[1] = g.tiles;
    plan[2] = g.stile;
    plan[3] = g.stiles;
    plan[4] = g.vec;
    plan[5] = (dims[0] + 1) * dims[1] * (12 * dims[4] + 8 * dims[2] * dims[3]);
    return 0;
}

static int lagr_rows(const int64_t* t_d, int64_t k, int64_t S, int64_t B, int64_t Hh, int64_t Ww, int64_t row0) {
    if (k < 1 || row0 < 0 || row0 + k > S + 1) return -1;
    if (t_d && (t_d[1] < 0 || t_d[0] < t_d[1] + 2)) return -1;
    if (t_d && (t_d[0] >= (1ll << 31) || k * B * Hh * Ww * t_d[0] >= (1ll << 40))) return -2;
    return 0;
}

extern "C" int tmg_ens_lagr_advect(const void* rows, const int64_t* t_d, const void* a, const void* o, const void* prev, void* pos,
                                   void* exit, void* res, const int64_t* seeds, const float* hs, const int64_t* dims, hipStream_t st) {
    if (!dims || !seeds) return -3;
    const int64_t k = dims[0], S = dims[1], B = dims[2], Hh = dims[3], Ww = dims[4], row0 = dims[5], t_before = dims[6];
    LagrSeeds g;
    int rc = lagr_sizes(S, B, Hh, Ww, 1);
    if (rc == -1) return rc;
    if (lagr_seeds(seeds, Hh, Ww, g) != 0 || t_before < 0) return -1;
    const int rr = lagr_rows(t_d, k, S, B, Hh, Ww, row0);
    if (rr == -1) return rr;
    if (rc != 0) return rc;
    if (rr != 0) return rr;
    if (t_before >= (1ll << 31)) return -2;
    if (!rows || !t_d || !a || !o || !prev || !pos || !exit || !hs || (g.R > 0 && !res)) return -3;
    LagrSteps h;
    for (int j = 0; j <= LAGR_MAXSUB; ++j) h.s[j] = hs[j];
    h.h = hs[LAGR_MAXSUB + 1], h.hh = hs[LAGR_MAXSUB + 2];
    const int64_t P = (int64_t)g.Gh * g.Gw;
    const LagrPlan pl = lagr_plan(Hh, Ww, P, 0);
    const dim3 grid((unsigned)pl.tiles, (unsigned)B, (unsigned)k);
    hipLaunchKernelGGL(ens_lagr_advect_kernel, grid, dim3(LAGR_THREADS), 0, st, (const float*)rows + t_d[1], (int)t_d[0], (const float*)a,
                       (const float*)o, (const float*)prev, (float*)pos, (int*)exit, (int*)res, g, h, (int)B, (int)Hh, (int)Ww, (int)row0,
                       (int)t_before - 1);
    TMG_CHECK_LAUNCH();
    return 0;
}

extern "C" int tmg_ens_lagr_store(const void* rows, const int64_t* t_d, const void* a, const void* o, void* prev, const int64_t* dims,
                                  hipStream_t st) {
    if (!dims) return -3;
    const int64_t k = dims[0], S = dims[1], B = dims[2], Hh = dims[3], Ww = dims[4], row0 = dims[5];
    int rc = lagr_sizes(S, B, Hh, Ww, 1);
    if (rc == -1) return rc;
    const int rr = lagr_rows(t_d, k, S, B, Hh, Ww, row0);
    if (rr == -1) return rr;
    if (rc != 0) return rc;
    if (rr != 0) return rr;
    if (!rows || !t_d || !a || !o || !prev) return -3;
    const LagrPlan pl = lagr_plan(Hh, Ww, 1, ((uintptr_t)prev & 15) == 0);
    const dim3 grid((unsigned)pl.stiles, (unsigned)B, (unsigned)k);
#define LAGR_LAUNCH(V_)                                                                                                                \
    hipLaunchKernelGGL((ens_lagr_store_kernel<V_>), grid, dim3(LAGR_THREADS), 0, st, (const float*)rows + t_d[1], (int)t_d[0],         \
                       (const float*)a, (const float*)o, (float*)prev, (int)B, (int)(Hh * Ww), (int)row0)
    if (pl.vec) LAGR_LAUNCH(1);
    else LAGR_LAUNCH(0);
#undef LAGR_LAUNCH
    TMG_CHECK_LAUNCH();
    return 0;
}

extern "C" int tmg_ens_lagr_finalize(const void* pos, const void* exit, const void* res, const double* fl, void* const* outs,
                                     const int64_t* seeds, const int64_t* dims, hipStream_t st) {
    if (!dims || !seeds) return -3;
    const int64_t S = dims[0], B = dims[1], Hh = dims[2], Ww = dims[3];
    LagrSeeds g;
    int rc = lagr_sizes(S, B, Hh, Ww, 1);
    if (rc == -1) return rc;
    if (lagr_seeds(seeds, Hh, Ww, g) != 0) return -1;
    if (fl) {
        for (int q = 0; q < 4; ++q)
            if (!(fl[q] > 0.0) || !(fl[q] <= 1.0e300)) return -1;
    }
    if (rc != 0) return rc;
    if (!pos || !exit || !fl || !outs || (g.R > 0 && !res)) return -3;
    LagrOuts o;
    for (int q = 0; q < LAGR_OUTS; ++q) o.p[q] = outs[q];
    for (int q = 0; q < 14; ++q)
        if (!o.p[q] && !(g.R == 0 && q >= 9 && q <= 11)) return -3;
    if ((o.p[14] != nullptr) != (o.p[15] != nullptr) || (o.p[14] != nullptr) != (o.p[16] != nullptr)) return -3;
    const LagrFl f = {fl[0], fl[1], fl[2], fl[3]};
    const int64_t P = (int64_t)g.Gh * g.Gw;
    const dim3 grid((unsigned)((P + LAGR_THREADS - 1) / LAGR_THREADS), (unsigned)B);
    hipLaunchKernelGGL(ens_lagr_finalize_kernel, grid, dim3(LAGR_THREADS), 0, st, (const float*)pos, (const int*)exit, (const int*)res, f, o,
                       g, (int)S, (int)B);
    TMG_CHECK_LAUNCH();
    return 0;
}
