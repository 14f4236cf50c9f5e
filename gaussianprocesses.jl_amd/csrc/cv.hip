// cv.hip — cross-validation on the device (src/crossvalidation.jl): logp_LOO + dlogpdθ_LOO (:50-175), predict_CVfold + logp_CVfold
// (:180-248), dlogpdθ_CVfold (:250-341).
//
// The reference forms Zj = inv(Σ) ∂K/∂θj and Zj inv(Σ) for every hyper-parameter: two dense N^3 products per parameter.  Here every
// parameter's derivative is ONE contraction tr(∂K/∂θj G) with a single N x N matrix G:
//     W = (K + σ²I)^-1,  α = W (y - m),  per fold V:  u_V = W_VV^-1 α_V,  B_V = W_VV^-1 + u_V u_V',
//     G = ½ (α b' + b α') - ½ W B W,  b = W u,   dlogp/dθj = tr(∂K/∂θj G),   dlogp/dlogσ = 2σ² tr(G)
// so the cost over gpmi_grad is the product W B W = S S' (S = W[:, F] M, M M' = B fold by fold: K = Σ s columns) and a few passes
// over N² / 2.  G2 is made to hold 2G: dmll_kernel (unchanged, alpha = 0, the "-K^-1" mode) counts the diagonal half and the strict
// lower part once, i.e. it returns ½ tr(G2 ∂K) = tr(G ∂K), and its trace slot tr(G2) = 2 tr(G) takes gpmi_grad's noise factor σ².
//
// Per fold, with W_VV = L L' (the fold's block of W, gathered with its sign fixed):
//     v = L^-1 α_V,  u_V = L^-T v,  ½ logdet W_VV = Σ log L_aa,  α_V' u_V = |v|²,
//     B_V = L^-T (I + v v') L^-1 = M M',   M = L^-T (I + γ v v') = L^-T + γ u_V v',   γ = 1 / (1 + sqrt(1 + |v|²))
// (I + γ v v')² = I + v v' for that γ), so no second factorisation of B_V is needed.  Folds of s <= 64 are factored one workgroup
// per fold in ONE launch (potf2_wg, potf2.h); folds of 65 .. 2048 are padded with the identity to the super-panel width above them and
// go through the factorisation's diagonal super-block factor + explicit inverse (super_factor_block, api.hip), one fold at a time.
// LOO needs none of it: W_ii is read off the diagonal, u_i = α_i / W_ii, B_ii = (1 + α_i u_i) / W_ii, S = W diag(sqrt(B_ii)).
#include <math.h>

#include <algorithm>
#include <string>
#include <vector>

#include "common.h"
#include "chol.h"
#include "mfma.h"
#include "potf2.h"

namespace gpmi {

template <typename T>
int super_factor_block(gpmi_ctx* c, T* blk, int64_t ld, int64_t w, T* linv, T* invdiag, T* lw, int64_t pivot_base);

namespace {

constexpr int CV_SMALL = 64;      // folds up to this size: one workgroup each (potf2_wg)
constexpr int64_t CV_PIV = 2048;  // a failing pivot p of fold f is reported as *info = (f + 1) CV_PIV + p: fold and pivot in one word
constexpr double LOG2PI = 1.8378770664093454836;

template <typename T>
__device__ __forceinline__ T wsym(const T* __restrict__ G, int64_t ld, int64_t i, int64_t j) {  // W_ij from the lower-stored tiles
    return i >= j ? G[i * ld + j] : G[j * ld + i];
}

// ---- folds of s <= 64: one 256-thread workgroup per fold --------------------------------------------------------------------------
// PRED: P receives W_VV^-1 (s x s, symmetric); otherwise M (row-major, M[r][c]).  ures[o + a] = u_V[a] in fold order, u[idx] = u_V.
template <typename T, bool PRED>
__global__ __launch_bounds__(256) void cv_small_kernel(const T* __restrict__ G2, int64_t ld, T sgn, const T* __restrict__ alpha,
                                                       const int64_t* __restrict__ idx, const int64_t* __restrict__ foff,
                                                       const int64_t* __restrict__ qoff, const int32_t* __restrict__ list,
                                                       int* __restrict__ info, T* __restrict__ invd, T* __restrict__ u,
                                                       T* __restrict__ ures, T* __restrict__ P, double* __restrict__ term) {
    __shared__ __attribute__((aligned(16))) double pool_d[POTF2_WG_POOL];
    __shared__ T sv[64], su[64];
    __shared__ T sg;
    constexpr int SLD = 65;
    T* const pool = reinterpret_cast<T*>(pool_d);
    T* const S = pool;
    T* const XT = S + 64 * SLD;
    const int tid = threadIdx.x;
    const int f = list[blockIdx.x];
    const int64_t o = foff[f], q = qoff[f];
    const int s = (int)(foff[f + 1] - o);
    for (int e = tid; e < 64 * 64; e += 256) {  // the fold's block of W (sign fixed), the identity below / right of it
        const int a = e >> 6, b = e & 63;
        S[a * SLD + b] = (a < s && b < s) ? sgn * wsym(G2, ld, idx[o + a], idx[o + b]) : (a == b ? T(1) : T(0));
    }
    __syncthreads();
    if (potf2_wg<T>(invd + (int64_t)blockIdx.x * 64, info, (int64_t)(f + 1) * CV_PIV, pool)) return;  // S = L, XT[n][k] = L^-1[k][n]
    if (tid < 64) {  // v = L^-1 alpha_V
        T acc = T(0);
        if (tid < s)
            for (int m = 0; m <= tid; ++m) acc += XT[m * SLD + tid] * alpha[idx[o + m]];
        sv[tid] = acc;
    }
    __syncthreads();
    if (tid < 64) {  // u = L^-T v
        T acc = T(0);
        if (tid < s)
            for (int k = tid; k < s; ++k) acc += XT[tid * SLD + k] * sv[k];
        su[tid] = acc;
    }
    __syncthreads();
    if (tid == 0) {  // fixed order: bit-reproducible
        double vv = 0.0, hl = 0.0;
        for (int a = 0; a < s; ++a) {
            vv += (double)sv[a] * (double)sv[a];
            hl += log((double)S[a * SLD + a]);
        }
        term[f] = -0.5 * s * LOG2PI + hl - 0.5 * vv;
        sg = (T)(1.0 / (1.0 + sqrt(1.0 + vv)));
    }
    __syncthreads();
    if (tid < s) {
        u[idx[o + tid]] = su[tid];
        ures[o + tid] = su[tid];
    }
    const T g = sg;
    for (int e = tid; e < s * s; e += 256) {
        const int r = e / s, cc = e - r * s;
        T val;
        if constexpr (PRED) {  // (L^-T L^-1)[r][c] = Σ_k L^-1[k][r] L^-1[k][c]
            val = T(0);
            for (int k = r > cc ? r : cc; k < s; ++k) val += XT[r * SLD + k] * XT[cc * SLD + k];
        } else {
            val = XT[r * SLD + cc] + g * su[r] * sv[cc];
        }
        P[q + e] = val;
    }
}

// ---- folds of 65 .. 2048: gather into the padded block, then (after the factor) the vectors and M ----------------------------------
template <typename T>
__global__ void cv_gather_kernel(const T* __restrict__ G2, int64_t ld, T sgn, const int64_t* __restrict__ idx, int s, T* __restrict__ blk,
                                 int64_t w) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= w * w) return;
    const int64_t a = e / w, b = e - a * w;
    blk[e] = (a < s && b < s) ? sgn * wsym(G2, ld, idx[a], idx[b]) : (a == b ? T(1) : T(0));
}

// one 1024-thread workgroup: lw = L^-1 of the padded block (row-major, leading dimension w), invd = 1 / L_aa
template <typename T>
__global__ __launch_bounds__(1024) void cv_large_vec_kernel(const T* __restrict__ lw, int64_t w, int s, const T* __restrict__ invd,
                                                            const T* __restrict__ alpha, const int64_t* __restrict__ idx, int f,
                                                            T* __restrict__ u, T* __restrict__ ures, T* __restrict__ vbuf,
                                                            double* __restrict__ term, T* __restrict__ gam) {
    __shared__ T sv[2048];
    __shared__ double r1[1024], r2[1024];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (int k = wv; k < s; k += 16) {  // v_k = Σ_{m <= k} L^-1[k][m] α_m: one wave per row
        T acc = T(0);
        for (int m = lane; m <= k; m += 64) acc += lw[(int64_t)k * w + m] * alpha[idx[m]];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
        if (lane == 0) sv[k] = acc;
    }
    __syncthreads();
    double vv = 0.0, hl = 0.0;
    for (int a = tid; a < s; a += 1024) {  // u_a = Σ_{k >= a} L^-1[k][a] v_k
        T acc = T(0);
        for (int k = a; k < s; ++k) acc += lw[(int64_t)k * w + a] * sv[k];
        ures[a] = acc;
        u[idx[a]] = acc;
        vbuf[a] = sv[a];
        vv += (double)sv[a] * (double)sv[a];
        hl -= log((double)invd[a]);
    }
    r1[tid] = vv;
    r2[tid] = hl;
    __syncthreads();
    for (int k = 512; k > 0; k >>= 1) {
        if (tid < k) {
            r1[tid] += r1[tid + k];
            r2[tid] += r2[tid + k];
        }
        __syncthreads();
    }
    if (tid == 0) {
        term[f] = -0.5 * s * LOG2PI + r2[0] - 0.5 * r1[0];
        *gam = (T)(1.0 / (1.0 + sqrt(1.0 + r1[0])));
    }
}

// M[r][c] = L^-1[c][r] + γ u_r v_c  (PRED: the transpose L^-T alone, the operand of the covariance product)
template <typename T>
__global__ void cv_large_m_kernel(const T* __restrict__ lw, int64_t w, int s, const T* __restrict__ ures, const T* __restrict__ vbuf,
                                  const T* __restrict__ gam, T* __restrict__ out, int64_t ldo, bool plain) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (int64_t)s * s) return;
    const int64_t r = e / s, c = e - r * s;
    const T t = lw[c * w + r];
    out[r * ldo + c] = plain ? t : t + (*gam) * ures[r] * vbuf[c];
}

// the super-block factor of a large fold runs with pivot base 0: put the fold into a pivot it reported
__global__ void cv_tag_info_kernel(int* info, int f) {
    const int v = *info;
    if (v > 0 && v <= CV_PIV) *info = (int)((f + 1) * CV_PIV) + v;
}

template <typename T>
__global__ void cv_copy_block_kernel(const T* __restrict__ src, int64_t lds, int s, T* __restrict__ dst) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (int64_t)s * s) return;
    const int64_t r = e / s, c = e - r * s;
    dst[e] = src[r * lds + c];
}

// ---- LOO: W_ii, u, sqrt(B_ii), the per-point terms ---------------------------------------------------------------------------------
template <typename T>
__global__ void cv_loo_prep_kernel(const T* __restrict__ G2, int64_t ld, T sgn, const T* __restrict__ alpha, int64_t n, int64_t npad,
                                   T* __restrict__ u, T* __restrict__ cs, double* __restrict__ term) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npad) return;
    if (i >= n) {
        u[i] = T(0);
        cs[i] = T(0);
        return;
    }
    const T wii = sgn * G2[i * ld + i];
    const T ui = alpha[i] / wii;
    u[i] = ui;
    cs[i] = sqrt((T(1) + alpha[i] * ui) / wii);
    term[i] = -0.5 * LOG2PI + 0.5 * log((double)wii) - 0.5 * (double)alpha[i] * (double)ui;
}

// b = W u from the lower tiles, one 64-row block per workgroup: the row part (j <= i) along the rows, the rest (j > i) down the
// columns, 64 contiguous entries per row; fixed order throughout
template <typename T>
__global__ __launch_bounds__(256) void cv_symv_kernel(const T* __restrict__ G2, int64_t ld, T sgn, const T* __restrict__ u, int64_t n,
                                                      T* __restrict__ b) {
    __shared__ T rp[64], cp[4][64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t i0 = (int64_t)blockIdx.x * 64;
    for (int rr = 0; rr < 16; ++rr) {
        const int64_t i = i0 + wv * 16 + rr;
        T acc = T(0);
        if (i < n)
            for (int64_t j = lane; j <= i; j += 64) acc += G2[i * ld + j] * u[j];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
        if (lane == 0) rp[wv * 16 + rr] = acc;
    }
    const int64_t ic = i0 + lane;
    T acc = T(0);
    if (ic < n)
        for (int64_t j = i0 + wv; j < n; j += 4)
            if (j > ic) acc += G2[j * ld + ic] * u[j];
    cp[wv][lane] = acc;
    __syncthreads();
    if (tid < 64 && i0 + tid < n) b[i0 + tid] = sgn * (rp[tid] + ((cp[0][tid] + cp[1][tid]) + (cp[2][tid] + cp[3][tid])));
}

// LOO: S[i][j] = W_ij sqrt(B_jj), the whole npad x npad square (zero outside n x n); a 64 x 64 tile per workgroup, the tiles above
// the diagonal transposed through LDS from their mirror image
template <typename T>
__global__ __launch_bounds__(256) void cv_loo_s_kernel(const T* __restrict__ G2, int64_t ld, const T* __restrict__ cs, int64_t n,
                                                       T* __restrict__ S) {
    __shared__ T t[64][65];
    const int tid = threadIdx.x;
    const int64_t I = blockIdx.y, J = blockIdx.x;
    const int64_t sr = (I >= J ? I : J) * 64, sc = (I >= J ? J : I) * 64;
    for (int e = tid; e < 64 * 64; e += 256) {
        const int r = e >> 6, c = e & 63;
        t[r][c] = (sr + r < n && sc + c < n) ? G2[(sr + r) * ld + sc + c] : T(0);
    }
    __syncthreads();
    for (int e = tid; e < 64 * 64; e += 256) {
        const int r = e >> 6, c = e & 63;
        const int64_t i = I * 64 + r, j = J * 64 + c;
        const T val = (i >= j) ? t[r][c] : t[c][r];
        S[i * ld + j] = (i < n && j < n) ? val * cs[j] : T(0);
    }
}

// folds: S[i][o_f + c] = Σ_r W[i][V_r] M_f[r][c] for the tile (fold f, columns c0 .. c0 + 64) x (rows i0 .. i0 + 64)
template <typename T>
__global__ __launch_bounds__(256) void cv_fold_s_kernel(const T* __restrict__ G2, int64_t ld, const int64_t* __restrict__ idx,
                                                        const int64_t* __restrict__ foff, const int64_t* __restrict__ qoff,
                                                        const T* __restrict__ P, const int32_t* __restrict__ tiles, int64_t n,
                                                        T* __restrict__ S) {
    __shared__ T wt[64][65], mt[64][65];
    const int tid = threadIdx.x;
    const int f = tiles[2 * blockIdx.x], c0 = tiles[2 * blockIdx.x + 1];
    const int64_t o = foff[f], q = qoff[f];
    const int s = (int)(foff[f + 1] - o);
    const int cw = s - c0 < 64 ? s - c0 : 64;
    const int64_t i0 = (int64_t)blockIdx.y * 64;
    const int tr = tid >> 4, tc = tid & 15;  // rows tr + 16 k, columns tc + 16 m
    T acc[4][4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int m = 0; m < 4; ++m) acc[k][m] = T(0);
    for (int r0 = 0; r0 < s; r0 += 64) {
        const int rw = s - r0 < 64 ? s - r0 : 64;
        for (int e = tid; e < 64 * 64; e += 256) {
            const int a = e >> 6, b = e & 63;
            const int64_t i = i0 + a;
            wt[a][b] = (i < n && b < rw) ? wsym(G2, ld, i, idx[o + r0 + b]) : T(0);
            mt[a][b] = (a < rw && b < cw) ? P[q + (int64_t)(r0 + a) * s + c0 + b] : T(0);
        }
        __syncthreads();
        for (int r = 0; r < 64; ++r) {
            T wr[4], mr[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) wr[k] = wt[tr + 16 * k][r];
#pragma unroll
            for (int m = 0; m < 4; ++m) mr[m] = mt[r][tc + 16 * m];
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int m = 0; m < 4; ++m) acc[k][m] += wr[k] * mr[m];
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int c = tc + 16 * m;
            if (c < cw) S[(i0 + tr + 16 * k) * ld + o + c0 + c] = acc[k][m];  // rows >= n hold zeros (wt)
        }
}

// G2 (= -S S') += α b' + b α' on the lower tiles, i, j < n
template <typename T>
__global__ void cv_rank2_kernel(T* __restrict__ G2, int64_t ld, const T* __restrict__ alpha, const T* __restrict__ b, int64_t n) {
    const int64_t I = blockIdx.y, J = blockIdx.x;
    if (J > I) return;
    for (int e = threadIdx.x; e < 64 * 64; e += blockDim.x) {
        const int64_t i = I * 64 + (e >> 6), j = J * 64 + (e & 63);
        if (i < n && j <= i) G2[i * ld + j] += alpha[i] * b[j] + b[i] * alpha[j];
    }
}

__global__ __launch_bounds__(1024) void cv_sum_kernel(const double* __restrict__ v, int64_t m, double* __restrict__ out) {
    __shared__ double sh[1024];
    double a = 0.0;
    for (int64_t k = threadIdx.x; k < m; k += 1024) a += v[k];
    sh[threadIdx.x] = a;
    __syncthreads();
    for (int k = 512; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) sh[threadIdx.x] += sh[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = sh[0];
}

inline unsigned nblk(int64_t m, int t) { return (unsigned)((m + t - 1) / t); }

// carve the cross-validation scratch into aligned sections
struct Carve {
    char* base;
    int64_t off = 0;
    template <typename U>
    U* take(int64_t count) {
        U* p = reinterpret_cast<U*>(base + off);
        off += (count * (int64_t)sizeof(U) + 255) / 256 * 256;
        return p;
    }
};

}  // namespace

// mode: 0 = LOO gradient, 1 = fold predictions (resid_out / cov_out), 2 = fold gradient
template <typename T>
int cv_run(gpmi_gp* gp, int mode, const gpmi_kernel* k, const double* log_noise, int64_t n_folds, const int64_t* fold_ptr,
           const int64_t* fold_idx, double* logp_out, double* dkern_out, double* dnoise_out, void* resid_out, void* cov_out) {
    gpmi_ctx* c = gp->ctx;
    const int64_t n = gp->n, npad = gp->npad, ld = gp->ld;
    la_reset(c);
    int n_hyp = 0;
    if (mode != 1) {
        if (const int rc = upload_program(c, k, gp->d)) return rc;
        n_hyp = c->h_prog->n_hyp;
    }
    if (const int rc = alloc_grad_scratch(gp, (size_t)(npad * ld) * sizeof(T))) return rc;
    T* G1 = (T*)gp->g1;
    T* G2 = (T*)gp->g2;
    if (mode != 1) {  // the gradient kernel's block partials (gpmi_grad's buffer)
        const int64_t nt = (n + 63) / 64;
        const int64_t need = nt * nt * (n_hyp + 1) * (int64_t)sizeof(double);
        if (gp->gpart_cap < need) {
            if (gp->gpart) hipFree(gp->gpart);
            gp->gpart = nullptr;
            gp->gpart_cap = 0;
            GPMI_HIP(c, hipMalloc(&gp->gpart, (size_t)need));
            gp->gpart_cap = need;
        }
    }
    const bool loo = mode == 0;
    const int64_t nf = loo ? 0 : n_folds;
    const int64_t K = loo ? n : fold_ptr[nf];
    // the folds on the host: sizes, packed offsets, the small-fold list, the S tiles, the widest large fold
    std::vector<int64_t> qoff((size_t)nf + 1, 0);
    std::vector<int32_t> small, tiles;
    std::vector<int64_t> large;
    int64_t wmax = 0;
    for (int64_t f = 0; f < nf; ++f) {
        const int64_t s = fold_ptr[f + 1] - fold_ptr[f];
        qoff[(size_t)f + 1] = qoff[(size_t)f] + s * s;
        if (s <= CV_SMALL) {
            small.push_back((int32_t)f);
        } else {
            large.push_back(f);
            int64_t w = NB;
            while (w < s) w *= 2;
            wmax = std::max(wmax, w);
        }
        for (int64_t c0 = 0; c0 < s; c0 += 64) {
            tiles.push_back((int32_t)f);
            tiles.push_back((int32_t)c0);
        }
    }
    const int64_t Q = qoff[(size_t)nf];
    const int64_t nsm = (int64_t)small.size(), ntile = (int64_t)tiles.size() / 2;
    // scratch: idx, fold / packed offsets, lists, u, b, zeros, LOO sqrt(B_ii) or the fold's v, the packed blocks, the terms, logp
    const int64_t nterm = loo ? n : std::max<int64_t>(nf, 1);
    auto layout = [&](Carve& cv) {
        cv.take<int64_t>(std::max<int64_t>(K, 1));
        cv.take<int64_t>(nf + 1);
        cv.take<int64_t>(nf + 1);
        cv.take<int32_t>(std::max<int64_t>(nsm, 1));
        cv.take<int32_t>(std::max<int64_t>(2 * ntile, 1));
        cv.take<T>(npad);
        cv.take<T>(npad);
        cv.take<T>(npad);
        cv.take<T>(npad);
        cv.take<T>(std::max<int64_t>(K, 1));
        cv.take<T>(std::max<int64_t>(Q, 1));
        cv.take<T>(std::max<int64_t>(nsm, 1) * 64);
        cv.take<double>(nterm);
        cv.take<double>(4);
    };
    Carve probe{nullptr};
    layout(probe);
    if (const int rc = grow(c, &gp->cv, &gp->cv_cap, probe.off)) return rc;
    Carve cv{(char*)gp->cv};
    int64_t* d_idx = cv.take<int64_t>(std::max<int64_t>(K, 1));
    int64_t* d_foff = cv.take<int64_t>(nf + 1);
    int64_t* d_qoff = cv.take<int64_t>(nf + 1);
    int32_t* d_small = cv.take<int32_t>(std::max<int64_t>(nsm, 1));
    int32_t* d_tiles = cv.take<int32_t>(std::max<int64_t>(2 * ntile, 1));
    T* d_u = cv.take<T>(npad);
    T* d_b = cv.take<T>(npad);
    T* d_zero = cv.take<T>(npad);
    T* d_v = cv.take<T>(npad);
    T* d_ures = cv.take<T>(std::max<int64_t>(K, 1));
    T* d_P = cv.take<T>(std::max<int64_t>(Q, 1));
    T* d_invd = cv.take<T>(std::max<int64_t>(nsm, 1) * 64);
    double* d_term = cv.take<double>(nterm);
    double* d_out = cv.take<double>(4);
    // the padded block of one large fold: the block (factored in place; then the covariance product's output), L^-1, L^-T,
    // the 64 x 64 inverses, 1 / L_aa, gamma
    T *d_blk = nullptr, *d_lw = nullptr, *d_lt = nullptr, *d_linv = nullptr, *d_binvd = nullptr, *d_gam = nullptr;
    if (wmax > 0) {
        const int64_t need = (3 * wmax * wmax + wmax * 64 + wmax + 64) * (int64_t)sizeof(T);
        if (const int rc = grow(c, &gp->cvblk, &gp->cvblk_cap, need)) return rc;
        d_blk = (T*)gp->cvblk;
        d_lw = d_blk + wmax * wmax;
        d_lt = d_lw + wmax * wmax;
        d_linv = d_lt + wmax * wmax;
        d_binvd = d_linv + wmax * 64;
        d_gam = d_binvd + wmax;
    }
    if (nf > 0) {
        GPMI_HIP(c, hipMemcpyAsync(d_idx, fold_idx, (size_t)K * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
        GPMI_HIP(c, hipMemcpyAsync(d_foff, fold_ptr, (size_t)(nf + 1) * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
        GPMI_HIP(c, hipMemcpyAsync(d_qoff, qoff.data(), (size_t)(nf + 1) * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
        if (nsm) GPMI_HIP(c, hipMemcpyAsync(d_small, small.data(), (size_t)nsm * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        if (ntile) GPMI_HIP(c, hipMemcpyAsync(d_tiles, tiles.data(), (size_t)(2 * ntile) * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        GPMI_HIP(c, hipStreamSynchronize(c->stream));  // the host vectors may go after this
    }
    GPMI_HIP(c, hipMemsetAsync(d_u, 0, (size_t)(4 * npad) * sizeof(T), c->stream));  // u, b, zeros, v (adjacent sections)
    GPMI_HIP(c, hipMemsetAsync(c->d_info, 0, sizeof(int), c->stream));
    const T* alpha = (const T*)gp->alpha;
    {
        ProfScope ps(c, GPMI_PROF_SOLVE, 2.0 * (double)npad * (double)npad * (double)npad / 3.0);
        const T sgn = build_kinv<T>(gp) ? T(-1) : T(1);
        // ---- the folds' blocks of W: factor, inverse, v, u, M (or W_VV^-1), the logp terms ----
        if (loo) {
            hipLaunchKernelGGL(cv_loo_prep_kernel<T>, dim3(nblk(npad, 256)), dim3(256), 0, c->stream, G2, ld, sgn, alpha, n, npad, d_u, d_v,
                               d_term);
        } else {
            if (nsm) {
                if (mode == 1)
                    hipLaunchKernelGGL((cv_small_kernel<T, true>), dim3((unsigned)nsm), dim3(256), 0, c->stream, G2, ld, sgn, alpha, d_idx, d_foff,
                                       d_qoff, d_small, c->d_info, d_invd, d_u, d_ures, d_P, d_term);
                else
                    hipLaunchKernelGGL((cv_small_kernel<T, false>), dim3((unsigned)nsm), dim3(256), 0, c->stream, G2, ld, sgn, alpha, d_idx, d_foff,
                                       d_qoff, d_small, c->d_info, d_invd, d_u, d_ures, d_P, d_term);
            }
            for (const int64_t f : large) {
                const int64_t o = fold_ptr[f], s = fold_ptr[f + 1] - o;
                int64_t w = NB;
                while (w < s) w *= 2;
                hipLaunchKernelGGL(cv_gather_kernel<T>, dim3(nblk(w * w, 256)), dim3(256), 0, c->stream, G2, ld, sgn, d_idx + o, (int)s, d_blk, w);
                if (const int rc = super_factor_block<T>(c, d_blk, w, w, d_linv, d_binvd, d_lw, 0)) return rc;
                hipLaunchKernelGGL(cv_tag_info_kernel, dim3(1), dim3(1), 0, c->stream, c->d_info, (int)f);
                hipLaunchKernelGGL(cv_large_vec_kernel<T>, dim3(1), dim3(1024), 0, c->stream, d_lw, w, (int)s, d_binvd, alpha, d_idx + o, (int)f,
                                   d_u, d_ures + o, d_v, d_term, d_gam);
                if (mode == 1) {  // W_VV^-1 = L^-T L^-1: the transpose, one product, the s x s corner into the packed output
                    hipLaunchKernelGGL(cv_large_m_kernel<T>, dim3(nblk(w * w, 256)), dim3(256), 0, c->stream, d_lw, w, (int)w, d_ures + o, d_v,
                                       d_gam, d_lt, w, true);
                    launch_gemm_shape<T>(c, d_blk, w, d_lt, w, d_lt, w, w, w, w, TileShape{0, 0, 0, 0, 1, 0}, c->d_info, GEMM_OVERWRITE | GEMM_AUX);
                    hipLaunchKernelGGL(cv_copy_block_kernel<T>, dim3(nblk(s * s, 256)), dim3(256), 0, c->stream, d_blk, w, (int)s, d_P + qoff[(size_t)f]);
                } else {
                    hipLaunchKernelGGL(cv_large_m_kernel<T>, dim3(nblk(s * s, 256)), dim3(256), 0, c->stream, d_lw, w, (int)s, d_ures + o, d_v,
                                       d_gam, d_P + qoff[(size_t)f], s, false);
                }
            }
        }
        hipLaunchKernelGGL(cv_sum_kernel, dim3(1), dim3(1024), 0, c->stream, d_term, loo ? n : nf, d_out);
        if (mode != 1) {
            // ---- b = W u, S, G2 = -S S' + α b' + b α' (= 2G), the contraction ----
            hipLaunchKernelGGL(cv_symv_kernel<T>, dim3(nblk(n, 64)), dim3(256), 0, c->stream, G2, ld, sgn, d_u, n, d_b);
            const int64_t nt = npad / 64;
            int64_t Kp;
            if (loo) {
                hipLaunchKernelGGL(cv_loo_s_kernel<T>, dim3((unsigned)nt, (unsigned)nt), dim3(256), 0, c->stream, G2, ld, d_v, n, G1);
                Kp = npad;
            } else {
                Kp = (K + 63) / 64 * 64;
                GPMI_HIP(c, hipMemsetAsync(G1, 0, (size_t)(npad * ld) * sizeof(T), c->stream));
                hipLaunchKernelGGL(cv_fold_s_kernel<T>, dim3((unsigned)ntile, (unsigned)nt), dim3(256), 0, c->stream, G2, ld, d_idx, d_foff, d_qoff,
                                   d_P, d_tiles, n, G1);
            }
            // W B W = S S' (lower tiles), the K dimension chunked as gpmi_grad chunks K^-1: the first chunk writes -S S', the rest subtract
            const int64_t WK = c->grad_chunk;
            const bool chunked = WK > 0 && npad >= 4 * WK;
            if (!chunked) {
                launch_gemm_shape<T>(c, G2, ld, G1, ld, G1, ld, npad, npad, Kp, TileShape{0, 0, 1, 0, 1, 0}, nullptr, GEMM_OVERWRITE | GEMM_NEGOUT);
            } else {
                for (int64_t k0 = 0; k0 < Kp; k0 += WK) {
                    const int64_t kw = std::min<int64_t>(WK, Kp - k0);
                    launch_gemm_shape<T>(c, G2, ld, G1 + k0, ld, G1 + k0, ld, npad, npad, kw, TileShape{0, 0, 1, 0, 1, 0}, nullptr,
                                         k0 == 0 ? GEMM_OVERWRITE | GEMM_NEGOUT : 0);
                }
            }
            hipLaunchKernelGGL(cv_rank2_kernel<T>, dim3((unsigned)nt, (unsigned)nt), dim3(256), 0, c->stream, G2, ld, alpha, d_b, n);
            const int64_t nblocks = launch_dmll<T>(c, (const T*)gp->x, n, gp->d, d_zero, G2, ld, gp->gpart, n_hyp, true);
            launch_reduce_partials(c, gp->gpart, nblocks, n_hyp + 1, (double*)gp->g1);  // g1 is free again: result vector
        }
    }
    int h_info = 0;
    double h_logp = 0.0;
    std::vector<double> h((size_t)n_hyp + 1);
    GPMI_HIP(c, hipMemcpyAsync(&h_info, c->d_info, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    GPMI_HIP(c, hipMemcpyAsync(&h_logp, d_out, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (mode != 1) GPMI_HIP(c, hipMemcpyAsync(h.data(), gp->g1, h.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    GPMI_HIP(c, hipStreamSynchronize(c->stream));
    GPMI_HIP(c, hipGetLastError());
    if (h_info < 0) {
        c->err = "chain kernel: a dependency wait timed out (GPMI_CHAIN=0 selects the multi-launch chain)";
        return GPMI_EDEVICE;
    }
    if (h_info > 0) {
        const int64_t f = (h_info - 1) / CV_PIV - 1, p = (h_info - 1) % CV_PIV + 1;
        c->err = "cross-validation: the block of (K + noise)^-1 on fold " + std::to_string(f) + " is not positive definite (pivot " +
                 std::to_string(p) + ")";
        return GPMI_ENOTPD;
    }
    if (logp_out) *logp_out = h_logp;
    if (mode == 1) {
        if (resid_out) GPMI_HIP(c, hipMemcpy(resid_out, d_ures, (size_t)K * sizeof(T), hipMemcpyDeviceToHost));
        if (cov_out) GPMI_HIP(c, hipMemcpy(cov_out, d_P, (size_t)Q * sizeof(T), hipMemcpyDeviceToHost));
        return GPMI_OK;
    }
    if (dkern_out)
        for (int p = 0; p < n_hyp; ++p) dkern_out[p] = h[(size_t)p];
    if (dnoise_out) *dnoise_out = exp(2.0 * log_noise[0]) * h[(size_t)n_hyp];  // 2σ² tr(G): the trace slot holds tr(2G)
    return GPMI_OK;
}

template int cv_run<double>(gpmi_gp*, int, const gpmi_kernel*, const double*, int64_t, const int64_t*, const int64_t*, double*, double*,
                            double*, void*, void*);
template int cv_run<float>(gpmi_gp*, int, const gpmi_kernel*, const double*, int64_t, const int64_t*, const int64_t*, double*, double*,
                           double*, void*, void*);

}  // namespace gpmi
