// The scale-to-scale energy flux and the sub-filter stresses of sampled roll-outs and of the target (tmg_ops.EnsembleFlux /
// utils.modelPredFlux): the coarse-graining analysis with a box filter of width w pixels, tau_ij = bar(u_i u_j) - bar(u_i) bar(u_j) and
// Pi = -tau_ij d bar(u_i) / dx_j at every instant, summed over the timed steps.  Rows are the S members plus the target as row S.
//   ens_flux_accum_kernel   one block of 1024 threads (a pixel each) per tile of 32 x 32 pixels of one row of one case.  The order: with
//                           f_c = fl(a_c y_c), c = 0, 1 (u, v), r = w / 2, N = w^2, the box sums
//                             Sg_u, Sg_v, Sg_uu, Sg_uv, Sg_vv  of  f_u, f_v, fl(f_u f_u), fl(f_u f_v), fl(f_v f_v)
//                           are a row pass followed by a column pass, both from the centre outwards:
//                             s_0 = g[0],  s_j = fl(fl(s_{j-1} + g[-j]) + g[+j]),  j = 1 .. r
//                           (row pass: g along W; column pass: g the row sums, along H).  Then
//                             Q_uu = fl(fl(N Sg_uu) - fl(Sg_u Sg_u)),  Q_uv = fl(fl(N Sg_uv) - fl(Sg_u Sg_v)),  Q_vv likewise     (N^2 tau)
//                             Sx, Sy = tmg_sobel3's combination (tmg_field.h, which says why it is written out here) of the three
//                             column / row differences of the box sums Sg_u, Sg_v
//                             A = fl(fl(Q_uu Sx Sg_u) + fl(Q_uv Sx Sg_v)),  B = fl(fl(Q_uv Sy Sg_u) + fl(Q_vv Sy Sg_v))
//                             Pi_s = -fl(fl(A kx) + fl(B ky)),  kx = 1 / (8 dx N^3), ky = 1 / (8 dy N^3) (fp32 tables from the host)
//                           and the planes of raw [S + 1][B][L][7][HW] are  0: A, 1: B, 2: fl(Pi_s Pi_s), 3: [Pi_s < 0], 4..6: Q_uu, Q_uv,
//                           Q_vv,  raw = fl(raw + term), one addition per timed step in step order; the first timed step stores the
//                           term, so the state needs no memset.  A pixel is valid for w when r + 1 <= h <= H - 2 - r and the same
//                           in w (box and stencil ring inside the field); the planes of an invalid pixel are neither read nor
//                           written.  Every operation is rounded on its own (no contraction): a float32 host mirror gives the same
//                           bits.  No running-window subtraction and no summed-area table: both cancel where tau is small.  A
//                           pixel's sums depend on its neighbourhood alone, never on the tile it fell in, and an element of raw
//                           is touched by one thread once per call: no atomics, no partial sums, bitwise reproducible.
//                           LDS: the block stages f_u, f_v of the tile plus the halo r_max + 1 (F, rows of pitch 66), keeps the five
//                           row sums of every staged row at the tile's 34 columns (tile plus its one-pixel ring; R, pitch 34) and
//                           extends them from width to width (the taps r_{l-1} + 1 .. r_l continue the same chain), and per width
//                           runs the column pass of Sg_u, Sg_v for the 34 x 34 ring (G, pitch 34: what the stencils read) and of
//                           the three products for the pixel itself, in registers.
//                           The pitches: every pass walks a LINEAR index over 34-wide rows with one lane per index, so the 32
//                           lanes of a ds_read_b32 group (banks = dword address mod 32) sit on 32 consecutive indices.  R and G have
//                           pitch 34, so their address IS the index (plus j 34 for the column pass's tap j, the same for all
//                           lanes): 32 consecutive dwords, 32 banks.  F has pitch 66 = 34 + 32: a group that straddles two rows
//                           of the index reads dword index + 32 in the second row, the same bank as its index: again 32 banks.  A
//                           pitch of 32 + 2 halo (dense) would put the second row's lanes 2 r_max dwords off and pile them onto the
//                           banks of the first row's lanes.  The pixel phase has a wave on two whole tile rows (32 lanes each).
//                           All 7 plane loads of a pixel are issued before the column pass, its 7 stores come last.
//   ens_flux_terms_kernel   once per mini-batch: one thread per (case, width, pixel) loops over the S + 1 rows; in fp64 it forms
//                           Pi = -(raw_0 kx + raw_1 ky) / T, the temporal std sqrt(max(raw_2 / T - Pi^2, 0)), the backscatter fraction
//                           raw_3 / T, tau = raw_4..6 / (N^2 T), a Welford mean / M2 over the members in member order, and one
//                           partial per wave (xor butterfly, a fixed order) of Pi and of (tau_uu + tau_vv) / 2 over the valid
//                           pixels; ens_flux_curve_kernel folds the partials in wave order.
#include "tmg_common.h"
#include "tmglow_hip.h"
#include "tmglow_hip_flux.h"

#define FLUX_MAXS 1024
#define FLUX_MAXL 8
#define FLUX_THREADS 1024
#define FLUX_FIN_THREADS 256
#define FLUX_Q 7
#define FLUX_TH 32
#define FLUX_TW 32
#define FLUX_PR (FLUX_TW + 2)
#define FLUX_PF (FLUX_PR + 32)
#define FLUX_PXT (FLUX_TH * FLUX_TW / FLUX_THREADS)                          // pixels per thread
#define FLUX_LDS_STATIC_MAX (64 * 1024)

struct FluxPlan {
    int64_t halo, org, nty, ntx, rows, lds, optin;
    unsigned long long rpack;                                                  // the radii, 8 bits each
};

// L in 1 .. 8 odd widths in 3 .. 33, strictly increasing, each <= min(H, W) - 2 (one valid pixel at least)
static int flux_widths(int64_t Hh, int64_t Ww, int64_t L, const int64_t* widths) {
    if (L < 1 || L > FLUX_MAXL || Hh < 5 || Ww < 5) return -1;
    if (!widths) return -3;
    const int64_t lim = (Hh < Ww ? Hh : Ww) - 2;
    for (int64_t l = 0; l < L; ++l) {
        const int64_t w = widths[l];
        if (w < 3 || w > 33 || w % 2 == 0 || w > lim || (l > 0 && w <= widths[l - 1])) return -1;
    }
    return 0;
}

// A function of (H, W, widths) alone.  The tiles cover the valid region of the smallest width, rows and columns org .. H - 1 - org.
static FluxPlan flux_plan(int64_t Hh, int64_t Ww, int64_t L, const int64_t* widths) {
    FluxPlan g;
    g.rpack = 0;
    for (int64_t l = 0; l < L; ++l) g.rpack |= (unsigned long long)(widths[l] / 2) << (8 * l);
    g.halo = widths[L - 1] / 2 + 1;
    g.org = widths[0] / 2 + 1;
    g.nty = (Hh - 2 * g.org + FLUX_TH - 1) / FLUX_TH;
    g.ntx = (Ww - 2 * g.org + FLUX_TW - 1) / FLUX_TW;
    g.rows = FLUX_TH + 2 * g.halo;
    g.lds = (2 * g.rows * FLUX_PF + 5 * g.rows * FLUX_PR + 2 * (FLUX_TH + 2) * FLUX_PR) * (int64_t)sizeof(float);
    g.optin = g.lds > FLUX_LDS_STATIC_MAX ? 1 : 0;
    return g;
}

__global__ __launch_bounds__(FLUX_THREADS) void ens_flux_accum_kernel(const float* __restrict__ y, int ps, const float* __restrict__ a,
                                                                      const float* __restrict__ kk, float* __restrict__ raw,
                                                                      unsigned long long rpack, int L, int B, int Hh, int Ww, int row0,
                                                                      int first, int ntx, int halo, int org) {
#pragma clang fp contract(off)
    extern __shared__ float flux_lds[];
    const int rows = FLUX_TH + 2 * halo, cols = FLUX_TW + 2 * halo;
    float* Fu = flux_lds;
    float* Fv = Fu + rows * FLUX_PF;
    float* R = Fv + rows * FLUX_PF;                                            // 5 planes of rows x 34
    float* G = R + 5 * rows * FLUX_PR;                                         // 2 planes of 34 x 34
    const int RP = rows * FLUX_PR, GP = (FLUX_TH + 2) * FLUX_PR;
    const int tid = threadIdx.x, s = blockIdx.y, b = blockIdx.z;
    const int ty0 = org + ((int)blockIdx.x / ntx) * FLUX_TH, tx0 = org + ((int)blockIdx.x % ntx) * FLUX_TW;
    const size_t hw = (size_t)Hh * Ww;
    const float a0 = a[b * 2], a1 = a[b * 2 + 1];
    const float* yp = y + ((size_t)s * B + b) * hw * ps;
    // stage f_u, f_v of the tile plus halo; 0 outside the field (no valid pixel reads it)
    for (int i = tid; i < rows * cols; i += FLUX_THREADS) {
        const int ry = i / cols, rx = i - ry * cols;
        const int fh = ty0 - halo + ry, fw = tx0 - halo + rx;
        float u = 0.f, v = 0.f;
        if (fh >= 0 && fh < Hh && fw >= 0 && fw < Ww) {
            const float* q = yp + ((size_t)fh * Ww + fw) * ps;
            u = a0 * q[0];
            v = a1 * q[1];
        }
        Fu[ry * FLUX_PF + rx] = u;
        Fv[ry * FLUX_PF + rx] = v;
    }
    __syncthreads();
    int rprev = 0;
    for (int l = 0; l < L; ++l) {
        const int r = (int)((rpack >> (8 * l)) & 0xffull);
        // the row pass, extended from the last width's: element i is owned by the same thread at every width
        for (int i = tid; i < RP; i += FLUX_THREADS) {
            const int ry = i / FLUX_PR, x = i - ry * FLUX_PR;
            const float* fu = Fu + ry * FLUX_PF + x + halo - 1;               // ring column x is staged column x + halo - 1
            const float* fv = Fv + ry * FLUX_PF + x + halo - 1;
            float s0, s1, s2, s3, s4;
            if (l == 0) {
                const float u = fu[0], v = fv[0];
                s0 = u, s1 = v, s2 = u * u, s3 = u * v, s4 = v * v;
            } else {
                s0 = R[i], s1 = R[RP + i], s2 = R[2 * RP + i], s3 = R[3 * RP + i], s4 = R[4 * RP + i];
            }
            for (int j = rprev + 1; j <= r; ++j) {
                const float um = fu[-j], vm = fv[-j], up = fu[j], vp = fv[j];
                const float uum = um * um, uvm = um * vm, vvm = vm * vm, uup = up * up, uvp = up * vp, vvp = vp * vp;
                s0 = (s0 + um) + up;
                s1 = (s1 + vm) + vp;
                s2 = (s2 + uum) + uup;
                s3 = (s3 + uvm) + uvp;
                s4 = (s4 + vvm) + vvp;
            }
            R[i] = s0, R[RP + i] = s1, R[2 * RP + i] = s2, R[3 * RP + i] = s3, R[4 * RP + i] = s4;
        }
        __syncthreads();
        // the column pass of Sg_u, Sg_v for the tile and its ring
        for (int i = tid; i < GP; i += FLUX_THREADS) {
            const int py = i / FLUX_PR, x = i - py * FLUX_PR;
            const float* c = R + (py + halo - 1) * FLUX_PR + x;               // ring row py is staged row py + halo - 1
            float s0 = c[0], s1 = c[RP];
            for (int j = 1; j <= r; ++j) {
                s0 = (s0 + c[-j * FLUX_PR]) + c[j * FLUX_PR];
                s1 = (s1 + c[RP - j * FLUX_PR]) + c[RP + j * FLUX_PR];
            }
            G[i] = s0, G[GP + i] = s1;
        }
        __syncthreads();
        // the pixels: FLUX_PXT per thread, a wave on two whole tile rows
        const int w = 2 * r + 1;
        const float Nf = (float)(w * w), kx = kk[2 * l], ky = kk[2 * l + 1];
        const int tx = tid & 31, fw = tx0 + tx;
        bool ok[FLUX_PXT];
        float* rp[FLUX_PXT];
        float old[FLUX_PXT][FLUX_Q];
#pragma unroll
        for (int n = 0; n < FLUX_PXT; ++n) {
            const int fh = ty0 + (tid >> 5) + (FLUX_THREADS / 32) * n;
            ok[n] = fh >= r + 1 && fh <= Hh - 2 - r && fw >= r + 1 && fw <= Ww - 2 - r;
            rp[n] = raw + ((((size_t)(row0 + s) * B + b) * L + l) * FLUX_Q) * hw + ((size_t)fh * Ww + fw);
            if (ok[n] && !first) {                                             // all 7 loads first
#pragma unroll
                for (int q = 0; q < FLUX_Q; ++q) old[n][q] = rp[n][q * hw];
            }
        }
#pragma unroll
        for (int n = 0; n < FLUX_PXT; ++n) {
            if (!ok[n]) continue;
            const int ty = (tid >> 5) + (FLUX_THREADS / 32) * n;
            const float* c = R + 2 * RP + (ty + halo) * FLUX_PR + tx + 1;
            float suu = c[0], suv = c[RP], svv = c[2 * RP];
            for (int j = 1; j <= r; ++j) {
                suu = (suu + c[-j * FLUX_PR]) + c[j * FLUX_PR];
                suv = (suv + c[RP - j * FLUX_PR]) + c[RP + j * FLUX_PR];
                svv = (svv + c[2 * RP - j * FLUX_PR]) + c[2 * RP + j * FLUX_PR];
            }
            const float* gu = G + (ty + 1) * FLUX_PR + tx + 1;
            const float* gv = gu + GP;
            const float su = gu[0], sv = gv[0];
            const float nuu = Nf * suu, nuv = Nf * suv, nvv = Nf * svv;
            const float puu = su * su, puv = su * sv, pvv = sv * sv;
            const float quu = nuu - puu, quv = nuv - puv, qvv = nvv - pvv;
            const int dn = FLUX_PR, up = -FLUX_PR;                            // row h + 1, row h - 1
            const float xu0 = gu[up + 1] - gu[up - 1], xu1 = gu[1] - gu[-1], xu2 = gu[dn + 1] - gu[dn - 1];
            const float xv0 = gv[up + 1] - gv[up - 1], xv1 = gv[1] - gv[-1], xv2 = gv[dn + 1] - gv[dn - 1];
            const float sxu = (xu0 + 2.f * xu1) + xu2, sxv = (xv0 + 2.f * xv1) + xv2;
            const float yu0 = gu[dn - 1] - gu[up - 1], yu1 = gu[dn] - gu[up], yu2 = gu[dn + 1] - gu[up + 1];
            const float yv0 = gv[dn - 1] - gv[up - 1], yv1 = gv[dn] - gv[up], yv2 = gv[dn + 1] - gv[up + 1];
            const float syu = (yu0 + 2.f * yu1) + yu2, syv = (yv0 + 2.f * yv1) + yv2;
            const float a_0 = quu * sxu, a_1 = quv * sxv, b_0 = quv * syu, b_1 = qvv * syv;
            const float A = a_0 + a_1, Bq = b_0 + b_1;
            const float ak = A * kx, bk = Bq * ky;
            const float pi = -(ak + bk);
            float t[FLUX_Q];
            t[0] = A, t[1] = Bq, t[2] = pi * pi, t[3] = pi < 0.f ? 1.f : 0.f, t[4] = quu, t[5] = quv, t[6] = qvv;
#pragma unroll
            for (int q = 0; q < FLUX_Q; ++q) t[q] = first ? t[q] : old[n][q] + t[q];
#pragma unroll
            for (int q = 0; q < FLUX_Q; ++q) rp[n][q * hw] = t[q];             // all 7 stores last
        }
        rprev = r;
        __syncthreads();                                                       // R and G are rewritten for the next width
    }
}

// the outputs of tmg_ens_flux_terms, in the order of its table `outs`
enum { FO_FLUX_MEAN, FO_FLUX_STD, FO_TARGET_FLUX, FO_TSTD_MEAN, FO_TARGET_TSTD, FO_BS_MEAN, FO_BS_STD, FO_TARGET_BS, FO_SGS_MEAN, FO_SGS_STD,
       FO_TARGET_SGS, FO_MEMBER_FLUX, FO_FLUX_CURVE, FO_SGS_CURVE, FO_N };
struct FluxOuts {
    float* p[FO_FLUX_CURVE];
};

__global__ __launch_bounds__(FLUX_FIN_THREADS) void ens_flux_terms_kernel(const float* __restrict__ raw, const double* __restrict__ k64,
                                                                          FluxOuts o, double* __restrict__ part, unsigned long long rpack,
                                                                          int S, int B, int L, int Hh, int Ww, int Tn, int NWv) {
#pragma clang fp contract(off)
    const int HW = Hh * Ww;
    const long long p = (long long)blockIdx.x * FLUX_FIN_THREADS + threadIdx.x;
    const int b = blockIdx.y, l = blockIdx.z;
    const int r = (int)((rpack >> (8 * l)) & 0xffull);
    const bool live = p < HW;                                                  // (no early return: the wave sums need every lane)
    const int h = live ? (int)(p / Ww) : 0, w = live ? (int)(p - (long long)h * Ww) : 0;
    const bool valid = live && h >= r + 1 && h <= Hh - 2 - r && w >= r + 1 && w <= Ww - 2 - r;
    const size_t hw = (size_t)HW;
    const double T = (double)Tn, kx = k64[2 * l], ky = k64[2 * l + 1];
    const double Nn = (double)((2 * r + 1) * (2 * r + 1)), n2t = (Nn * Nn) * T;
    const double nanv = __builtin_nan("");
    const int wv = (int)blockIdx.x * (FLUX_FIN_THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    double mean[6], m2[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) mean[i] = 0.0, m2[i] = 0.0;
    const size_t po = ((size_t)b * L + l) * hw + (size_t)p;                    // [B][L][HW]
    for (int row = 0; row <= S; ++row) {
        double v[6];                                                           // Pi, tstd, backscatter, tau_uu, tau_uv, tau_vv
        if (valid) {
            const float* rp = raw + ((((size_t)row * B + b) * L + l) * FLUX_Q) * hw + (size_t)p;
            const double sa = (double)rp[0], sb = (double)rp[hw], s2 = (double)rp[2 * hw], cn = (double)rp[3 * hw];
            const double pi = -((sa * kx + sb * ky) / T);
            const double var = s2 / T - pi * pi;
            v[0] = pi;
            v[1] = sqrt(var < 0.0 ? 0.0 : var);
            v[2] = cn / T;
#pragma unroll
            for (int i = 0; i < 3; ++i) v[3 + i] = (double)rp[(4 + i) * hw] / n2t;
        } else {
#pragma unroll
            for (int i = 0; i < 6; ++i) v[i] = nanv;
        }
        const double cp = wave_sum(valid ? v[0] : 0.0), ce = wave_sum(valid ? 0.5 * (v[3] + v[5]) : 0.0);
        if (lane == 0) {
            double* pp = part + ((((size_t)b * (S + 1) + row) * L + l) * 2) * NWv + wv;
            pp[0] = cp;
            pp[NWv] = ce;
        }
        if (!live) continue;
        if (row < S) {
            const double rn = 1.0 / (double)(row + 1);
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                const double d = v[i] - mean[i];
                mean[i] = mean[i] + d * rn;
                m2[i] = m2[i] + d * (v[i] - mean[i]);
            }
            if (o.p[FO_MEMBER_FLUX]) o.p[FO_MEMBER_FLUX][(((size_t)b * S + row) * L + l) * hw + (size_t)p] = (float)v[0];
        } else {
            o.p[FO_TARGET_FLUX][po] = (float)v[0];
            o.p[FO_TARGET_TSTD][po] = (float)v[1];
            o.p[FO_TARGET_BS][po] = (float)v[2];
#pragma unroll
            for (int i = 0; i < 3; ++i) o.p[FO_TARGET_SGS][(((size_t)b * L + l) * 3 + i) * hw + (size_t)p] = (float)v[3 + i];
        }
    }
    if (!live) return;
    const double rs = 1.0 / (double)S;
    double sd[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) sd[i] = sqrt((m2[i] < 0.0 ? 0.0 : m2[i]) * rs);   // (a NaN m2 stays NaN: the invalid region)
    o.p[FO_FLUX_MEAN][po] = (float)mean[0], o.p[FO_FLUX_STD][po] = (float)sd[0];
    o.p[FO_TSTD_MEAN][po] = (float)mean[1];
    o.p[FO_BS_MEAN][po] = (float)mean[2], o.p[FO_BS_STD][po] = (float)sd[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        o.p[FO_SGS_MEAN][(((size_t)b * L + l) * 3 + i) * hw + (size_t)p] = (float)mean[3 + i];
        o.p[FO_SGS_STD][(((size_t)b * L + l) * 3 + i) * hw + (size_t)p] = (float)sd[3 + i];
    }
}

// One thread per (case, row, width): the wave partials folded in wave order, over the number of valid pixels.
__global__ __launch_bounds__(FLUX_FIN_THREADS) void ens_flux_curve_kernel(const double* __restrict__ part, float* __restrict__ flux_curve,
                                                                          float* __restrict__ sgs_curve, unsigned long long rpack, int n, int L,
                                                                          int Hh, int Ww, int NWv) {
#pragma clang fp contract(off)
    const long long i = (long long)blockIdx.x * FLUX_FIN_THREADS + threadIdx.x;    // ((b (S + 1) + row) L + l)
    if (i >= n) return;
    const int r = (int)((rpack >> (8 * (int)(i % L))) & 0xffull);
    const double cnt = (double)(Hh - 2 - 2 * r) * (double)(Ww - 2 - 2 * r);
    const double* pp = part + (size_t)i * 2 * NWv;
    double sp = 0.0, se = 0.0;
    for (int k = 0; k < NWv; ++k) sp = sp + pp[k], se = se + pp[NWv + k];
    flux_curve[i] = (float)(sp / cnt);
    sgs_curve[i] = (float)(se / cnt);
}

static int flux_sizes(int64_t S, int64_t B, int64_t Hh, int64_t Ww, int64_t L) {
    if (S < 1 || B < 1 || Hh < 5 || Ww < 5 || L < 1 || L > FLUX_MAXL) return -1;
    if (S > FLUX_MAXS || B > 65535 || Hh >= (1ll << 31) || Ww >= (1ll << 31) || Hh * Ww >= (1ll << 31) - 4 * FLUX_THREADS ||
        (S + 1) * B * L * FLUX_Q * Hh * Ww >= (1ll << 40))
        return -2;
    return 0;
}

extern "C" int tmg_ens_flux_plan(const int64_t* dims, const int64_t* widths, int64_t* plan) {
    if (!dims) return -3;
    const int64_t S = dims[0], B = dims[1], Hh = dims[2], Ww = dims[3], L = dims[4];
    const int rc = flux_sizes(S, B, Hh, Ww, L);
    if (rc == -1) return rc;
    const int rw = flux_widths(Hh, Ww, L, widths);
    if (rw == -1) return rw;
    if (rc != 0) return rc;
    if (rw != 0 || !plan) return -3;
    const FluxPlan g = flux_plan(Hh, Ww, L, widths);
    plan[0] = FLUX_TH;
    plan[1] = FLUX_TW;
    plan[2] = g.halo;
    plan[3] = g.nty;
    plan[4] = g.ntx;
    plan[5] = g.lds;
    plan[6] = g.optin;
    plan[7] = g.nty * g.ntx * B;
    return 0;
}

extern "C" int tmg_ens_flux_accum(const void* rows, const int64_t* t_d, const void* a, const void* kk, void* raw, const int64_t* widths,
                                  const int64_t* dims, hipStream_t st) {
    if (!dims) return -3;
    const int64_t k = dims[0], S = dims[1], B = dims[2], Hh = dims[3], Ww = dims[4], row0 = dims[5], t_before = dims[6], L = dims[7];
    int rc = flux_sizes(S, B, Hh, Ww, L);
    if (rc == -1) return rc;
    if (k < 1 || row0 < 0 || row0 + k > S + 1 || t_before < 0) return -1;
    if (t_d && (t_d[1] < 0 || t_d[0] < t_d[1] + 2)) return -1;
    const int rw = flux_widths(Hh, Ww, L, widths);
    if (rw == -1) return rw;
    if (rc != 0) return rc;
    if (t_d && (t_d[0] >= (1ll << 31) || k * B * Hh * Ww * t_d[0] >= (1ll << 40))) return -2;
    if (rw != 0 || !rows || !t_d || !a || !kk || !raw) return -3;
    const FluxPlan g = flux_plan(Hh, Ww, L, widths);
    const float* yr = (const float*)rows + t_d[1];
    if (g.optin) TMG_LDS_OPTIN(ens_flux_accum_kernel);
    const dim3 grid((unsigned)(g.nty * g.ntx), (unsigned)k, (unsigned)B);
    hipLaunchKernelGGL(ens_flux_accum_kernel, grid, dim3(FLUX_THREADS), (size_t)g.lds, st, yr, (int)t_d[0], (const float*)a, (const float*)kk,
                       (float*)raw, g.rpack, (int)L, (int)B, (int)Hh, (int)Ww, (int)row0, (int)(t_before == 0), (int)g.ntx, (int)g.halo,
                       (int)g.org);
    TMG_CHECK_LAUNCH();
    return 0;
}

extern "C" int tmg_ens_flux_terms(const void* raw, const void* k64, void* const* outs, void* ws, const int64_t* widths, const int64_t* dims,
                                  hipStream_t st) {
    if (!dims) return -3;
    const int64_t S = dims[0], B = dims[1], Hh = dims[2], Ww = dims[3], T = dims[4], L = dims[5];
    int rc = flux_sizes(S, B, Hh, Ww, L);
    if (rc == -1) return rc;
    if (T < 1) return -1;
    const int rw = flux_widths(Hh, Ww, L, widths);
    if (rw == -1) return rw;
    if (rc != 0) return rc;
    if (T >= (1ll << 31)) return -2;
    if (rw != 0 || !raw || !k64 || !outs || !ws) return -3;
    for (int i = 0; i < FO_N; ++i)
        if (i != FO_MEMBER_FLUX && !outs[i]) return -3;                        // (member_flux is optional)
    const FluxPlan g = flux_plan(Hh, Ww, L, widths);
    FluxOuts o;
    float** op = &o.p[FO_FLUX_MEAN];
    for (int i = 0; i < 12; ++i) op[i] = (float*)outs[i];
    const int64_t nb = (Hh * Ww + FLUX_FIN_THREADS - 1) / FLUX_FIN_THREADS, NWv = nb * (FLUX_FIN_THREADS / 64);
    hipLaunchKernelGGL(ens_flux_terms_kernel, dim3((unsigned)nb, (unsigned)B, (unsigned)L), dim3(FLUX_FIN_THREADS), 0, st, (const float*)raw,
                       (const double*)k64, o, (double*)ws, g.rpack, (int)S, (int)B, (int)L, (int)Hh, (int)Ww, (int)T, (int)NWv);
    TMG_CHECK_LAUNCH();
    const int64_t n = B * (S + 1) * L;
    hipLaunchKernelGGL(ens_flux_curve_kernel, dim3((unsigned)((n + FLUX_FIN_THREADS - 1) / FLUX_FIN_THREADS)), dim3(FLUX_FIN_THREADS), 0, st,
                       (const double*)ws, (float*)outs[FO_FLUX_CURVE], (float*)outs[FO_SGS_CURVE], g.rpack, (int)n, (int)L, (int)Hh, (int)Ww, (int)NWv);
    TMG_CHECK_LAUNCH();
    return 0;
}
