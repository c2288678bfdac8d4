// Spectral skill of sampled roll-outs against the target (tmg_ops.EnsembleSpectralSkill / utils.modelPredSpectralSkill): per wavenumber
// shell the power P, the co-spectrum X with the target and the error power D of every member and of the ensemble-mean field
// (definitions: include/tmglow_hip_xspec.h).  The 2-D DFT is tmg_spectrum.hip's: the row pass is tmg_spec_rows, called unchanged with
// unit tables on the field this file's prep kernel forms; the column pass below has spec_cols_kernel's product, lane for lane and k
// for k (tmg_dft.h states it and why it is written out in both kernels), so that a member that equals the target gives the target's bits.
//   xspec_prep_kernel   one thread per element of [B][H][W][2]: f = u fmaf(out_std, y, out_mu) - M of channels 0 and 1 of every image
//                       of the NHWC chunk (run-time pixel stride) into the dense buffer f [k*B][H][W][2]; the members' f added in
//                       member order into fsum (the step's first chunk stores); mode 3 writes fbar = fsum / S instead
//   xspec_cols_kernel   column transform Z = F_H Y of a 16-column tile (Y panel in LDS), Z into an LDS tile.  Target mode: Z also goes
//                       planar to zt, and P is summed per shell.  Cross mode: the dead Y panel is re-staged with the target's Z tile and
//                       one thread per shell walks the shell's list, forming P, X, D of each mode on the fly into three sums
//   xspec_accum_kernel  one thread per (case, quantity, shell): the tiles' partial sums in tile order, the chunk's members in member
//                       order into the step sums and into each member's time sums; the target at the step's first chunk, the mean
//                       field and the step's outputs at its last
// Every element of every state is owned by one thread per launch and every sum has a fixed order: the same inputs give the same bits
// for every chunking.  No data-dependent addressing: the shell lists are host-built and checked by the caller.
#include "tmg_dft.h"
#include "tmg_field.h"
#include "tmglow_hip_xspec.h"

#define XS_MAXSHELLS 8192
#define XS_MAXS 1024

// mode 0: f only (the target); 1: members, fsum stored; 2: members, fsum loaded, added to, stored; 3: f = fsum / S (no y)
__global__ __launch_bounds__(256) void xspec_prep_kernel(const float* __restrict__ y, int ps, const float* __restrict__ u,
                                                         const float* __restrict__ out_mu, const float* __restrict__ out_std,
                                                         const float* __restrict__ cen, float* __restrict__ f, float* __restrict__ fsum,
                                                         int k, int B, int HW, int mode, float members) {
#pragma clang fp contract(off)
    const size_t n = (size_t)B * HW * 2;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    if (mode == 3) {
        f[e] = fsum[e] / members;
        return;
    }
    const int c = (int)(e & 1);
    const size_t pix = e >> 1;                       // b * HW + p
    const int b = (int)(pix / HW);
    const int p = (int)(pix - (size_t)b * HW);
    const float sc = u ? u[b * 2 + c] : 1.f;
    const float mu = out_mu[c], sd = out_std[c];
    const float m = cen ? cen[((size_t)b * 2 + c) * HW + p] : 0.f;
    float s = mode == 2 ? fsum[e] : 0.f;
    for (int j = 0; j < k; ++j) {
        const float q = y[((size_t)j * B * HW + pix) * ps + c];
        float v = tmg_unnorm_fma(q, sc, sd, mu);
        if (cen) v = v - m;                          // one separate rounding
        f[(size_t)j * n + e] = v;
        s = (mode == 1 && j == 0) ? v : s + v;
    }
    if (mode) fsum[e] = s;
}

extern "C" int tmg_ens_xspec_plan(const int64_t* dims, int64_t* out) {
    if (!dims || !out) return -3;
    const int64_t k = dims[0], B = dims[1], Hh = dims[2], Ww = dims[3], NK = dims[4];
    if (k < 1 || B < 1 || NK < 1) return -1;
    if (!tmg_dft_side_ok(Hh) || !tmg_dft_side_ok(Ww)) return -1;
    if (k > XS_MAXS || 3 * B > 65535 || k * B > 65535 || NK > XS_MAXSHELLS) return -2;
    const int64_t QT = Ww / 16, img = Hh * Ww;
    out[0] = (B * img * 2 + 255) / 256;              // prep grid: one thread per element of [B][H][W][2]
    out[1] = QT;                                     // cols grid x: the 16-column tiles
    out[2] = k * B;                                  // cols grid y: the images
    out[3] = 256 * Hh;                               // cols LDS bytes: Y panel [2][H][16] and Z tile [2][H][16]
    out[4] = (NK + 255) / 256;                       // accum grid x
    out[5] = 3 * B;                                  // accum grid y: (case, quantity of (P, X, D))
    out[6] = 256;                                    // threads of every block
    out[7] = k * B * img * 2;                        // floats of f, and of the row pass's planar workspace
    out[8] = k * B * QT * 3 * NK;                    // floats of the cross mode's partial sums [k*B][QT][3][NK]
    out[9] = B * img * 2;                            // floats of zt, and of fsum
    out[10] = B * QT * NK;                           // floats of the target mode's partial sums [B][QT][NK]
    return 0;
}

extern "C" int tmg_ens_xspec_prep(const void* y, const int64_t* y_d, const void* u, const void* out_mu, const void* out_std,
                                  const void* center, void* f, void* fsum, const int64_t* dims, hipStream_t st) {
    if (!dims) return -3;
    const int64_t k = dims[0], B = dims[1], Hh = dims[2], Ww = dims[3], C = dims[4], mode = dims[5], S = dims[6], f_floats = dims[7];
    int64_t plan[11];
    const int64_t pd[5] = {k, B, Hh, Ww, 1};
    const int rc = tmg_ens_xspec_plan(pd, plan);
    if (rc) return rc;
    if (mode < 0 || mode > 3 || S < 1) return -1;
    if (S > XS_MAXS) return -2;
    if (mode == 3 && k != 1) return -1;
    if (mode != 3) {
        if (!y_d) return -3;
        if (C < 2 || C > 4 || y_d[0] < C || y_d[1] < 0 || y_d[1] + C > y_d[0]) return -1;
        if (k * B * Hh * Ww * y_d[0] >= (1ll << 40)) return -2;
        if (!y || !out_mu || !out_std) return -3;
    }
    if (!f || (mode && !fsum)) return -3;
    if (f_floats < plan[7]) return -4;
    hipLaunchKernelGGL(xspec_prep_kernel, dim3((unsigned)plan[0]), dim3(256), 0, st,
                       mode == 3 ? (const float*)nullptr : (const float*)y + y_d[1], mode == 3 ? 0 : (int)y_d[0], (const float*)u,
                       (const float*)out_mu, (const float*)out_std, (const float*)center, (float*)f, (float*)fsum, (int)k, (int)B,
                       (int)(Hh * Ww), (int)mode, (float)S);
    TMG_CHECK_LAUNCH();
    return 0;
}

// LDS: the Y panel [2][H][16] (re, im), re-staged with the target's Z tile in cross mode; the Z tile [2][H][16].
// cross = 0: zt is written, part [img][QT][NK] = P.  cross = 1: zt is read (image img % B), part [img][QT][3][NK] = (P, X, D).
__global__ __launch_bounds__(256) void xspec_cols_kernel(const float* __restrict__ ft, const float* __restrict__ yw, size_t plane,
                                                         const int* __restrict__ perm, const int* __restrict__ offs,
                                                         float* __restrict__ zt, size_t zplane, float* __restrict__ part, int B, int Hh,
                                                         int Ww, int NK, float scale, int cross) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int img = blockIdx.y, qt = blockIdx.x, QT = gridDim.x;
    const int HP = Hh * 16;
    float* zre = lds + 2 * HP;
    float* zim = lds + 3 * HP;
    const float* ysrc = yw + (size_t)img * Hh * Ww + qt * 16;
    for (int i = threadIdx.x; i < HP; i += 256) {
        const size_t g = (size_t)(i >> 4) * Ww + (i & 15);
        lds[i] = ysrc[g];
        lds[HP + i] = ysrc[plane + g];
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, l = threadIdx.x & 63, l16 = l & 15, lq = l >> 4;
    const float* br = lds + lq * 16 + l16;
    const float* bi = br + HP;
    const size_t th = (size_t)Hh * Hh;
    float* ztile = zt + (size_t)(img % B) * Hh * Ww + qt * 16;
    for (int pt = wave; pt < (Hh >> 4); pt += 4) {
        const float* fr = ft + (size_t)lq * Hh + pt * 16 + l16;
        const float* fi = fr + th;
        f32x4 zr = {0.f, 0.f, 0.f, 0.f}, zi = {0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < Hh; k0 += 16)        // H is a multiple of 16; the column product of tmg_dft.h
#pragma unroll
        for (int k = k0; k < k0 + 16; k += 4) {
            const float a_r = fr[(size_t)k * Hh], a_i = fi[(size_t)k * Hh];
            const float b_r = br[k * 16], b_i = bi[k * 16];
            zr = __builtin_amdgcn_mfma_f32_16x16x4f32(a_r, b_r, zr, 0, 0, 0);
            zi = __builtin_amdgcn_mfma_f32_16x16x4f32(a_r, b_i, zi, 0, 0, 0);
            zr = __builtin_amdgcn_mfma_f32_16x16x4f32(-a_i, b_i, zr, 0, 0, 0);
            zi = __builtin_amdgcn_mfma_f32_16x16x4f32(a_i, b_r, zi, 0, 0, 0);
        }
        const int row = pt * 16 + lq * 4;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            zre[(row + r) * 16 + l16] = zr[r];
            zim[(row + r) * 16 + l16] = zi[r];
        }
        if (!cross) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                ztile[(size_t)(row + r) * Ww + l16] = zr[r];
                ztile[zplane + (size_t)(row + r) * Ww + l16] = zi[r];
            }
        }
    }
    __syncthreads();                                 // every wave is done with the Y panel
    if (cross) {
        for (int i = threadIdx.x; i < HP; i += 256) {
            const size_t g = (size_t)(i >> 4) * Ww + (i & 15);
            lds[i] = ztile[g];
            lds[HP + i] = ztile[zplane + g];
        }
        __syncthreads();
    }
    // shell sums of the tile in list order: positions of[s] .. of[s + 1] - 1 of pm hold the tile indices (p * 16 + column) of shell s
    const int* pm = perm + (size_t)qt * HP;
    const int* of = offs + (size_t)qt * (NK + 1);
    if (cross) {
        float* o = part + ((size_t)img * QT + qt) * 3 * NK;
        for (int s = threadIdx.x; s < NK; s += 256) {
            float aP = 0.f, aX = 0.f, aD = 0.f;
            const int i1 = of[s + 1];
            for (int i = of[s]; i < i1; ++i) {
                const int m = pm[i];
                const float vr = zre[m], vi = zim[m], tr = lds[m], ti = lds[HP + m];
                const float dr = vr - tr, di = vi - ti;
                aP += scale * (vr * vr + vi * vi);
                aX += scale * (vr * tr + vi * ti);
                aD += scale * (dr * dr + di * di);
            }
            o[s] = aP;
            o[NK + s] = aX;
            o[2 * NK + s] = aD;
        }
    } else {
        float* o = part + ((size_t)img * QT + qt) * NK;
        for (int s = threadIdx.x; s < NK; s += 256) {
            float aP = 0.f;
            const int i1 = of[s + 1];
            for (int i = of[s]; i < i1; ++i) {
                const int m = pm[i];
                const float vr = zre[m], vi = zim[m];
                aP += scale * (vr * vr + vi * vi);
            }
            o[s] = aP;
        }
    }
}

extern "C" int tmg_ens_xspec_cols(const void* ft, const void* yw, const void* perm, const void* offs, void* zt, void* part,
                                  const int64_t* dims, const float* fl, hipStream_t st) {
    if (!dims || !fl) return -3;
    const int64_t n = dims[0], B = dims[1], Hh = dims[2], Ww = dims[3], NK = dims[4], cross = dims[5], yw_floats = dims[6],
                  zt_floats = dims[7], part_floats = dims[8];
    if (n < 1 || B < 1 || NK < 1 || (cross != 0 && cross != 1)) return -1;
    if (!tmg_dft_side_ok(Hh) || !tmg_dft_side_ok(Ww)) return -1;
    if (n % B || (!cross && n != B)) return -1;
    if (!(fl[0] > 0.f) || !(fl[0] <= 3.0e38f)) return -1;
    if (n > 65535 || NK > XS_MAXSHELLS) return -2;
    if (!ft || !yw || !perm || !offs || !zt || !part) return -3;
    const int64_t plane = n * Hh * Ww, zplane = B * Hh * Ww, QT = Ww / 16;
    if (yw_floats < 2 * plane || zt_floats < 2 * zplane || part_floats < n * QT * NK * (cross ? 3 : 1)) return -4;
    const size_t smem = (size_t)4 * Hh * 16 * sizeof(float);
    TMG_LDS_OPTIN(xspec_cols_kernel);
    hipLaunchKernelGGL(xspec_cols_kernel, dim3((unsigned)QT, (unsigned)n), dim3(256), smem, st, (const float*)ft, (const float*)yw,
                       (size_t)plane, (const int*)perm, (const int*)offs, (float*)zt, (size_t)zplane, (float*)part, (int)B, (int)Hh,
                       (int)Ww, (int)NK, fl[0], (int)cross);
    TMG_CHECK_LAUNCH();
    return 0;
}

// The tiles' partial sums of one quantity in tile order.
__device__ __forceinline__ float xs_fold(const float* __restrict__ pp, int QT, size_t stride) {
    float a = 0.f;
    for (int t = 0; t < QT; ++t) a += pp[(size_t)t * stride];
    return a;
}

// The first timed step stores, later ones add.
__device__ __forceinline__ void xs_time(float* __restrict__ p, float v, int t_before) { *p = t_before > 0 ? *p + v : v; }

// flags & 1: the step is timed; flags & 2: the step's last chunk.  The step's first chunk (n_before == 0) holds the target's sums.
// One thread per (case, quantity q of (P, X, D), shell); the thread of P also folds the target's P.
__global__ __launch_bounds__(256) void xspec_accum_kernel(const float* __restrict__ part, const float* __restrict__ part_t,
                                                          const float* __restrict__ part_b, float* __restrict__ step,
                                                          float* __restrict__ tpow, float* __restrict__ sum_out,
                                                          float* __restrict__ bar_out, float* __restrict__ tmem, float* __restrict__ ttgt,
                                                          float* __restrict__ tbar, int k, int B, int NK, int QT, int S, int Tk, int t,
                                                          int n_before, int m0, int t_before, int flags) {
#pragma clang fp contract(off)
    const int s = blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y / 3, q = blockIdx.y - 3 * b;
    if (s >= NK) return;
    const size_t qs = (size_t)q * NK + s;
    const size_t si = (size_t)b * 3 * NK + qs;
    float a = n_before > 0 ? step[si] : 0.f;
    for (int j = 0; j < k; ++j) {
        const float v = xs_fold(part + (size_t)(j * B + b) * QT * 3 * NK + qs, QT, (size_t)3 * NK);
        a += v;
        if (flags & 1) xs_time(tmem + ((size_t)b * S + m0 + j) * 3 * NK + qs, v, t_before);
    }
    if (n_before == 0 && q == 0) {
        const float v = xs_fold(part_t + (size_t)b * QT * NK + s, QT, (size_t)NK);
        tpow[((size_t)b * Tk + t) * NK + s] = v;
        if (flags & 1) xs_time(ttgt + (size_t)b * NK + s, v, t_before);
    }
    if (flags & 2) {
        const float v = xs_fold(part_b + (size_t)b * QT * 3 * NK + qs, QT, (size_t)3 * NK);
        const size_t oi = ((size_t)b * Tk + t) * 3 * NK + qs;
        bar_out[oi] = v;
        sum_out[oi] = a;
        if (flags & 1) xs_time(tbar + si, v, t_before);
    } else {
        step[si] = a;
    }
}

extern "C" int tmg_ens_xspec_accum(const void* part, const void* part_t, const void* part_b, void* step, void* tpow, void* sum_out,
                                   void* bar_out, void* tmem, void* ttgt, void* tbar, const int64_t* dims, hipStream_t st) {
    if (!dims) return -3;
    const int64_t k = dims[0], B = dims[1], NK = dims[2], QT = dims[3], S = dims[4], Tk = dims[5], t = dims[6], n_before = dims[7],
                  m0 = dims[8], t_before = dims[9], flags = dims[10];
    if (k < 1 || B < 1 || NK < 1 || QT < 1 || QT > TMG_DFT_MAXN / 16 || S < 1 || Tk < 1 || t < 0 || t >= Tk || n_before < 0 || m0 < 0
        || t_before < 0 || flags < 0 || flags > 3)
        return -1;
    if (m0 != n_before || m0 + k > S || ((flags & 2) != 0) != (m0 + k == S)) return -1;
    if (S > XS_MAXS || 3 * B > 65535 || k * B > 65535 || NK > XS_MAXSHELLS || B * Tk * 3 * NK >= (1ll << 40)) return -2;
    if (!part || !step) return -3;
    if (n_before == 0 && (!part_t || !tpow)) return -3;
    if ((flags & 2) && (!part_b || !sum_out || !bar_out)) return -3;
    if ((flags & 1) && (!tmem || (n_before == 0 && !ttgt) || ((flags & 2) && !tbar))) return -3;
    hipLaunchKernelGGL(xspec_accum_kernel, dim3((unsigned)((NK + 255) / 256), (unsigned)(3 * B)), dim3(256), 0, st, (const float*)part,
                       (const float*)part_t, (const float*)part_b, (float*)step, (float*)tpow, (float*)sum_out, (float*)bar_out,
                       (float*)tmem, (float*)ttgt, (float*)tbar, (int)k, (int)B, (int)NK, (int)QT, (int)S, (int)Tk, (int)t,
                       (int)n_before, (int)m0, (int)t_before, (int)flags);
    TMG_CHECK_LAUNCH();
    return 0;
}
