// Linear-SVM validation on the device: the solver of sklearn's SVC(C, kernel="linear") (libsvm C-SVC, one-vs-one) without its
// shrinking heuristic, which does not move the fixed point.  The f64 Gram matrix on v_mfma_f64_16x16x4_f64, one SMO workgroup per
// class pair with alpha / gradient / Gram diagonal in LDS, the per-pair weight vectors and the one-vs-one vote.
// See include/gm3d.h for the contracts.  Compiled with -ffp-contract=off: the SMO path matches the float64 restatement of the tests
// operation for operation.
#include "common.hpp"

using namespace gm3d;

namespace {

constexpr int SVM_MAX_N = 16384, SVM_MAX_D = 1024, SVM_MAX_CLS = 64, SVM_MAX_PAIR = 4096;
constexpr int SVM_MAX_P = SVM_MAX_CLS * (SVM_MAX_CLS - 1) / 2;
constexpr int GRAM_TILE = 64, GRAM_KC = 32, GRAM_PITCH = GRAM_KC + 1;
constexpr int SMO_THREADS = 256, SMO_WAVES = SMO_THREADS / 64, SMO_R = SVM_MAX_PAIR / SMO_THREADS;   // <= 16 rows per thread
constexpr double TAU = 1e-12;                 // libsvm's floor of a non-positive curvature
constexpr int PRED_ROWS = 8, PRED_THREADS = 256, PRED_WAVES = PRED_THREADS / 64;

typedef double f64x4 __attribute__((ext_vector_type(4)));

struct ClassStart {
    int v[SVM_MAX_CLS + 1];       // rows of class c: [v[c], v[c+1])
};

// ---- Gram matrix ------------------------------------------------------------------------------------------------------------
// One 64x64 tile of the lower triangle per workgroup, mirrored on store.  Four waves in 2x2, each a 32x32 block of 2x2 16x16 f64
// MFMAs; the operands pass through LDS as f64 in 32-column chunks (zero beyond n / d).  Only entries with i >= j are stored, each
// to both (i,j) and (j,i): K is exactly symmetric.  f32 products are exact in f64, so K differs from X.double() @ X.double().T only
// in the order of the sums.
__global__ __launch_bounds__(256) void svm_gram_kernel(const float* __restrict__ X, int n, int d, double* __restrict__ K) {
    __shared__ double sa[GRAM_TILE * GRAM_PITCH], sb[GRAM_TILE * GRAM_PITCH];
    const long long b = blockIdx.x;
    int ti = (int)((sqrt(8.0 * (double)b + 1.0) - 1.0) * 0.5);
    while ((long long)ti * (ti + 1) / 2 > b) --ti;
    while ((long long)(ti + 1) * (ti + 2) / 2 <= b) ++ti;
    const int tj = (int)(b - (long long)ti * (ti + 1) / 2);
    const int i0 = ti * GRAM_TILE, j0 = tj * GRAM_TILE;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
    f64x4 acc[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[x][y] = f64x4{0.0, 0.0, 0.0, 0.0};
    const int lr = tid >> 2, lc = (tid & 3) * 8;          // loader: tile row, first of its 8 columns
    const int ra = i0 + lr, rb = j0 + lr;
    for (int k0 = 0; k0 < d; k0 += GRAM_KC) {
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int k = k0 + lc + c;
            sa[lr * GRAM_PITCH + lc + c] = (ra < n && k < d) ? (double)X[(size_t)ra * d + k] : 0.0;
            sb[lr * GRAM_PITCH + lc + c] = (rb < n && k < d) ? (double)X[(size_t)rb * d + k] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < GRAM_KC; kk += 4) {
            const int k = kk + (lane >> 4);               // A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15]
            double a[2], bv[2];
#pragma unroll
            for (int x = 0; x < 2; ++x) {
                a[x] = sa[(32 * wr + 16 * x + (lane & 15)) * GRAM_PITCH + k];
                bv[x] = sb[(32 * wc + 16 * x + (lane & 15)) * GRAM_PITCH + k];
            }
#pragma unroll
            for (int x = 0; x < 2; ++x)
#pragma unroll
                for (int y = 0; y < 2; ++y) acc[x][y] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[x], bv[y], acc[x][y], 0, 0, 0);
        }
        __syncthreads();
    }
    // f64 C/D layout: column = lane & 15, row = (lane >> 4) + 4 * reg
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = i0 + 32 * wr + 16 * x + (lane >> 4) + 4 * r;
                const int j = j0 + 32 * wc + 16 * y + (lane & 15);
                if (i < n && j < n && i >= j) {
                    const double v = acc[x][y][r];
                    K[(size_t)i * n + j] = v;
                    K[(size_t)j * n + i] = v;
                }
            }
}

// ---- class pairs ------------------------------------------------------------------------------------------------------------
// Pair p in sklearn's order (0,1), (0,2), ..., (0,c-1), (1,2), ...: rows of s (y = +1) then rows of t (y = -1), in dataset order.
// `off` = the pair's first slot in the concatenated per-pair alpha array (the sum of n_s + n_t over the pairs before it).
struct Pair {
    int s, t, s0, ns, t0, nt;
    long long off;
};

__device__ Pair pair_of(int p, const ClassStart& cs, int ncls) {
    long long off = 0;
    int s = 0, rem = p;
    for (; s < ncls - 1; ++s) {
        const int cnt = ncls - 1 - s, ns = cs.v[s + 1] - cs.v[s];
        if (rem < cnt) break;
        off += (long long)cnt * ns + (cs.v[ncls] - cs.v[s + 1]);
        rem -= cnt;
    }
    Pair q;
    q.s = s;
    q.t = s + 1 + rem;
    q.s0 = cs.v[s];
    q.ns = cs.v[s + 1] - cs.v[s];
    q.t0 = cs.v[q.t];
    q.nt = cs.v[q.t + 1] - cs.v[q.t];
    q.off = off + (long long)rem * q.ns + (cs.v[q.t] - cs.v[s + 1]);
    return q;
}

// (v, k) beats (bv, bk): larger value, ties to the lower row.  A total order: the butterfly leaves the same winner in every lane.
__device__ __forceinline__ bool better(double v, int k, double bv, int bk) { return v > bv || (v == bv && k < bk); }

__device__ __forceinline__ void wave_best(double& v, int& k) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double ov = __shfl_xor(v, off, 64);
        const int ok = __shfl_xor(k, off, 64);
        if (better(ov, ok, v, k)) {
            v = ov;
            k = ok;
        }
    }
}

__device__ __forceinline__ double wave_maxd(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
    return v;
}

// ---- SMO ----------------------------------------------------------------------------------------------------------------------
// libsvm's Solver for one class pair: alpha = 0, G = -1; i = argmax over I_up of -yG (= Gmax); Fan-Chen-Lin second-order choice of j
// over I_low; stop when Gmax + max over I_low of yG < tol; the two-variable update with libsvm's clipping; G += Q_i dai + Q_j daj.
// Thread `tid` owns the pair rows k = tid + 256 r; it keeps K[i, k] and K[j, k] of the current working set in registers.
__global__ __launch_bounds__(SMO_THREADS) void svm_smo_kernel(const double* __restrict__ K, int n, int ncls, ClassStart cs, double C,
                                                              double tol, long long max_iter, double* __restrict__ alpha_out,
                                                              double* __restrict__ rho_out, int* __restrict__ iters_out,
                                                              int* __restrict__ capped) {
    extern __shared__ double lds[];
    __shared__ double red_v[2][SMO_WAVES], red_g2[SMO_WAVES], red_s[SMO_WAVES], red_ub[SMO_WAVES], red_lb[SMO_WAVES];
    __shared__ int red_k[2][SMO_WAVES], red_n[SMO_WAVES];
    const Pair q = pair_of(blockIdx.x, cs, ncls);
    const int m = q.ns + q.nt, ns = q.ns;
    double* al = lds;
    double* G = al + m;
    double* Kd = G + m;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double INF = __builtin_inf();
    auto grow = [&](int k) { return k < ns ? q.s0 + k : q.t0 + (k - ns); };

    for (int k = tid; k < m; k += SMO_THREADS) {
        al[k] = 0.0;
        G[k] = -1.0;
        const int g = grow(k);
        Kd[k] = K[(size_t)g * n + g];
    }
    __syncthreads();
    const long long cap = max_iter > 0 ? max_iter : (100LL * m > 10000000LL ? 100LL * m : 10000000LL);
    long long it = 0;
    bool hit_cap = false;
    double Ki[SMO_R], Kj[SMO_R];
    for (;;) {
        if (it >= cap) {
            hit_cap = true;
            break;
        }
        // i = argmax over I_up of -yG; Gmax2 = max over I_low of yG
        double upv = -INF, g2 = -INF;
        int upk = 0x7fffffff;
#pragma unroll
        for (int r = 0; r < SMO_R; ++r) {
            const int k = tid + SMO_THREADS * r;
            if (k < m) {
                const bool pos = k < ns;
                const double a = al[k], yg = pos ? G[k] : -G[k];
                const bool up = pos ? a < C : a > 0.0, low = pos ? a > 0.0 : a < C;
                if (up && better(-yg, k, upv, upk)) {
                    upv = -yg;
                    upk = k;
                }
                if (low) g2 = fmax(g2, yg);
            }
        }
        wave_best(upv, upk);
        g2 = wave_maxd(g2);
        if (lane == 0) {
            red_v[0][wave] = upv;
            red_k[0][wave] = upk;
            red_g2[wave] = g2;
        }
        __syncthreads();
        double Gmax = red_v[0][0], Gmax2 = red_g2[0];
        int i = red_k[0][0];
        for (int w = 1; w < SMO_WAVES; ++w) {
            if (better(red_v[0][w], red_k[0][w], Gmax, i)) {
                Gmax = red_v[0][w];
                i = red_k[0][w];
            }
            Gmax2 = fmax(Gmax2, red_g2[w]);
        }
        if (!(Gmax + Gmax2 >= tol)) break;           // also when I_up or I_low is empty (-inf)

        // j: over k in I_low with b = Gmax + y_k G_k > 0, the argmin of -b^2 / a (= argmax of b^2 / a), a = K_ii + K_kk - 2 K_ik
        const int gi = grow(i);
        const double Kii = Kd[i], yi = i < ns ? 1.0 : -1.0;
        const double* Kir = K + (size_t)gi * n;
        double jv = -INF;
        int jk = 0x7fffffff;
#pragma unroll
        for (int r = 0; r < SMO_R; ++r) {
            const int k = tid + SMO_THREADS * r;
            if (k < m) {
                Ki[r] = Kir[grow(k)];
                const bool pos = k < ns;
                const double a = al[k], yg = pos ? G[k] : -G[k];
                const bool low = pos ? a > 0.0 : a < C;
                if (low) {
                    const double bgap = Gmax + yg;
                    if (bgap > 0.0) {
                        double quad = Kii + Kd[k] - 2.0 * Ki[r];
                        if (quad <= 0.0) quad = TAU;
                        const double v = (bgap * bgap) / quad;
                        if (better(v, k, jv, jk)) {
                            jv = v;
                            jk = k;
                        }
                    }
                }
            }
        }
        wave_best(jv, jk);
        if (lane == 0) {
            red_v[1][wave] = jv;
            red_k[1][wave] = jk;
        }
        __syncthreads();
        int j = red_k[1][0];
        double jbest = red_v[1][0];
        for (int w = 1; w < SMO_WAVES; ++w)
            if (better(red_v[1][w], red_k[1][w], jbest, j)) {
                jbest = red_v[1][w];
                j = red_k[1][w];
            }
        if (j >= m) break;                             // no j with b > 0 (libsvm: Gmin_idx == -1)

        // the two-variable update (libsvm Solver::Solve), computed identically by every thread
        const int gj = grow(j);
        const double yj = j < ns ? 1.0 : -1.0, Kjj = Kd[j];
        const double Qij = yi * yj * K[(size_t)gi * n + gj];
        const double aio = al[i], ajo = al[j], Gi = G[i], Gj = G[j];
        double ai = aio, aj = ajo;
        if (yi != yj) {
            double quad = Kii + Kjj + 2.0 * Qij;
            if (quad <= 0.0) quad = TAU;
            const double delta = (-Gi - Gj) / quad, diff = ai - aj;
            ai += delta;
            aj += delta;
            if (diff > 0.0) {
                if (aj < 0.0) {
                    aj = 0.0;
                    ai = diff;
                }
            } else if (ai < 0.0) {
                ai = 0.0;
                aj = -diff;
            }
            if (diff > 0.0) {                         // diff > C_i - C_j with C_i == C_j
                if (ai > C) {
                    ai = C;
                    aj = C - diff;
                }
            } else if (aj > C) {
                aj = C;
                ai = C + diff;
            }
        } else {
            double quad = Kii + Kjj - 2.0 * Qij;
            if (quad <= 0.0) quad = TAU;
            const double delta = (Gi - Gj) / quad, sum = ai + aj;
            ai -= delta;
            aj += delta;
            if (sum > C) {
                if (ai > C) {
                    ai = C;
                    aj = sum - C;
                }
            } else if (aj < 0.0) {
                aj = 0.0;
                ai = sum;
            }
            if (sum > C) {
                if (aj > C) {
                    aj = C;
                    ai = sum - C;
                }
            } else if (ai < 0.0) {
                ai = 0.0;
                aj = sum;
            }
        }
        const double dai = ai - aio, daj = aj - ajo;
        const double* Kjr = K + (size_t)gj * n;
#pragma unroll
        for (int r = 0; r < SMO_R; ++r) {
            const int k = tid + SMO_THREADS * r;
            if (k < m) Kj[r] = Kjr[grow(k)];
        }
        __syncthreads();                               // every thread has read the old alpha_i, alpha_j, G_i, G_j
        if (tid == 0) {
            al[i] = ai;
            al[j] = aj;
        }
#pragma unroll
        for (int r = 0; r < SMO_R; ++r) {
            const int k = tid + SMO_THREADS * r;
            if (k < m) {
                const double yk = k < ns ? 1.0 : -1.0;
                const double qi = yi * yk * Ki[r], qj = yj * yk * Kj[r];
                G[k] = G[k] + (qi * dai + qj * daj);
            }
        }
        ++it;
        __syncthreads();
    }

    // rho (libsvm calculate_rho): the mean of yG over the free alpha, else the midpoint of [lb, ub]
    double sfree = 0.0, ub = INF, lb = -INF;
    int nfree = 0;
#pragma unroll
    for (int r = 0; r < SMO_R; ++r) {
        const int k = tid + SMO_THREADS * r;
        if (k < m) {
            const bool pos = k < ns;
            const double a = al[k], yg = pos ? G[k] : -G[k];
            if (a >= C) {
                if (pos) lb = fmax(lb, yg); else ub = fmin(ub, yg);
            } else if (a <= 0.0) {
                if (pos) ub = fmin(ub, yg); else lb = fmax(lb, yg);
            } else {
                ++nfree;
                sfree += yg;
            }
            alpha_out[q.off + k] = a;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        sfree += __shfl_xor(sfree, off, 64);
        nfree += __shfl_xor(nfree, off, 64);
        ub = fmin(ub, __shfl_xor(ub, off, 64));
        lb = fmax(lb, __shfl_xor(lb, off, 64));
    }
    if (lane == 0) {
        red_s[wave] = sfree;
        red_n[wave] = nfree;
        red_ub[wave] = ub;
        red_lb[wave] = lb;
    }
    __syncthreads();
    if (tid == 0) {
        double s = 0.0, u = INF, l = -INF;
        int nf = 0;
        for (int w = 0; w < SMO_WAVES; ++w) {
            s += red_s[w];
            nf += red_n[w];
            u = fmin(u, red_ub[w]);
            l = fmax(l, red_lb[w]);
        }
        rho_out[blockIdx.x] = nf > 0 ? s / nf : (u + l) / 2.0;
        iters_out[blockIdx.x] = (int)it;
        if (hit_cap) atomicAdd(capped, 1);
    }
}

// ---- weights and prediction ------------------------------------------------------------------------------------------------------
// w[p, c] = sum over the pair's rows k, in order, of (y_k alpha_k) * X[k, c], in f64.  Grid (P, ceil(d / 256)).
__global__ __launch_bounds__(256) void svm_weights_kernel(const float* __restrict__ X, int d, int ncls, ClassStart cs,
                                                          const double* __restrict__ alpha, double* __restrict__ w) {
    const Pair q = pair_of(blockIdx.x, cs, ncls);
    const int c = blockIdx.y * 256 + threadIdx.x;
    if (c >= d) return;
    double acc = 0.0;
    for (int k = 0; k < q.ns; ++k) acc += alpha[q.off + k] * (double)X[(size_t)(q.s0 + k) * d + c];
    for (int k = 0; k < q.nt; ++k) acc += -alpha[q.off + q.ns + k] * (double)X[(size_t)(q.t0 + k) * d + c];
    w[(size_t)blockIdx.x * d + c] = acc;
}

// PRED_ROWS test rows per workgroup: dec_p = w_p . x - rho_p for every pair (one wave per pair, lanes over columns, a fixed
// butterfly), a vote for s if dec > 0 else for t (integer LDS counts), then the first class with the most votes.
__global__ __launch_bounds__(PRED_THREADS) void svm_predict_kernel(const float* __restrict__ X, int m, int d, int ncls,
                                                                   const double* __restrict__ w, const double* __restrict__ rho,
                                                                   const long long* __restrict__ labels, long long* __restrict__ pred,
                                                                   unsigned long long* __restrict__ correct) {
    __shared__ float xs[PRED_ROWS * SVM_MAX_D];
    __shared__ int votes[PRED_ROWS * SVM_MAX_CLS];
    __shared__ unsigned char ps[SVM_MAX_P], pt[SVM_MAX_P];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row0 = blockIdx.x * PRED_ROWS;
    const int P = ncls * (ncls - 1) / 2;
    for (int e = tid; e < PRED_ROWS * d; e += PRED_THREADS) {
        const int r = e / d, c = e - r * d;
        xs[e] = row0 + r < m ? X[(size_t)(row0 + r) * d + c] : 0.0f;
    }
    for (int e = tid; e < PRED_ROWS * SVM_MAX_CLS; e += PRED_THREADS) votes[e] = 0;
    if (tid == 0) {
        int p = 0;
        for (int s = 0; s < ncls; ++s)
            for (int t = s + 1; t < ncls; ++t, ++p) {
                ps[p] = (unsigned char)s;
                pt[p] = (unsigned char)t;
            }
    }
    __syncthreads();
    for (int p = wave; p < P; p += PRED_WAVES) {
        double acc[PRED_ROWS];
#pragma unroll
        for (int r = 0; r < PRED_ROWS; ++r) acc[r] = 0.0;
        const double* wp = w + (size_t)p * d;
        for (int c = lane; c < d; c += 64) {
            const double wc = wp[c];
#pragma unroll
            for (int r = 0; r < PRED_ROWS; ++r) acc[r] += wc * (double)xs[r * d + c];
        }
#pragma unroll
        for (int r = 0; r < PRED_ROWS; ++r) {
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) acc[r] += __shfl_xor(acc[r], off, 64);
        }
        if (lane == 0) {
            const double rp = rho[p];
#pragma unroll
            for (int r = 0; r < PRED_ROWS; ++r)
                if (row0 + r < m) atomicAdd(&votes[r * SVM_MAX_CLS + (acc[r] - rp > 0.0 ? ps[p] : pt[p])], 1);
        }
    }
    __syncthreads();
    if (tid < PRED_ROWS && row0 + tid < m) {
        const int* v = votes + tid * SVM_MAX_CLS;
        int best = 0;
        for (int c = 1; c < ncls; ++c)
            if (v[c] > v[best]) best = c;
        pred[row0 + tid] = best;
        if (labels && (long long)best == labels[row0 + tid]) atomicAdd(correct, 1ull);
    }
}

// Host check of the class layout: 2 <= ncls <= 64, class_start[0] = 0 < ... (every class non-empty) ... = n, every pair <= 4096 rows.
int check_classes(int n, int ncls, const int* class_start, ClassStart* cs) {
    if (!class_start || n < 1 || ncls < 1) return GM3D_EINVAL;
    if (ncls < 2 || ncls > SVM_MAX_CLS || n > SVM_MAX_N) return GM3D_EUNSUPPORTED;
    if (class_start[0] != 0 || class_start[ncls] != n) return GM3D_EINVAL;
    for (int c = 0; c < ncls; ++c)
        if (class_start[c + 1] <= class_start[c]) return GM3D_EINVAL;
    int big1 = 0, big2 = 0;                                    // the two largest classes make the largest pair
    for (int c = 0; c < ncls; ++c) {
        const int sz = class_start[c + 1] - class_start[c];
        if (sz > big1) {
            big2 = big1;
            big1 = sz;
        } else if (sz > big2) {
            big2 = sz;
        }
    }
    if (big1 + big2 > SVM_MAX_PAIR) return GM3D_EUNSUPPORTED;
    for (int c = 0; c <= ncls; ++c) cs->v[c] = class_start[c];
    return GM3D_OK;
}

}  // namespace

extern "C" int gm3d_svm_gram(const float* X, int n, int d, double* K, gm3d_stream_t stream) {
    if (!X || !K || n < 1 || d < 1) return GM3D_EINVAL;
    if (n > SVM_MAX_N || d > SVM_MAX_D) return GM3D_EUNSUPPORTED;
    const long long T = (n + GRAM_TILE - 1) / GRAM_TILE;
    return launch_lds<svm_gram_kernel>(dim3((unsigned)(T * (T + 1) / 2)), dim3(256), 0, stream, X, n, d, K);
}

extern "C" int gm3d_svm_smo(const double* K, int n, int ncls, const int* class_start, double C, double tol, long long max_iter,
                            double* alpha, double* rho, int* iters, int* capped, gm3d_stream_t stream) {
    ClassStart cs;
    const int rc = check_classes(n, ncls, class_start, &cs);
    if (rc != GM3D_OK) return rc;
    if (!K || !alpha || !rho || !iters || !capped || !(C > 0.0) || !(tol > 0.0)) return GM3D_EINVAL;
    int mmax = 0;
    for (int s = 0; s < ncls; ++s)
        for (int t = s + 1; t < ncls; ++t) {
            const int m = cs.v[s + 1] - cs.v[s] + cs.v[t + 1] - cs.v[t];
            mmax = m > mmax ? m : mmax;
        }
    const size_t lds = (size_t)3 * mmax * sizeof(double);     // alpha, G, diag(K): 96 KiB at 4096 rows
    return launch_lds<svm_smo_kernel>(dim3(ncls * (ncls - 1) / 2), dim3(SMO_THREADS), lds, stream, K, n, ncls, cs, C, tol, max_iter,
                                      alpha, rho, iters, capped);
}

extern "C" int gm3d_svm_weights(const float* X, int n, int d, int ncls, const int* class_start, const double* alpha, double* w,
                                gm3d_stream_t stream) {
    ClassStart cs;
    const int rc = check_classes(n, ncls, class_start, &cs);
    if (rc != GM3D_OK) return rc;
    if (!X || !alpha || !w || d < 1) return GM3D_EINVAL;
    if (d > SVM_MAX_D) return GM3D_EUNSUPPORTED;
    return launch_lds<svm_weights_kernel>(dim3(ncls * (ncls - 1) / 2, (d + 255) / 256), dim3(256), 0, stream, X, d, ncls, cs, alpha, w);
}

extern "C" int gm3d_svm_predict(const float* X, int m, int d, int ncls, const double* w, const double* rho, const long long* labels,
                                long long* pred, long long* correct, gm3d_stream_t stream) {
    if (m < 0 || d < 1 || ncls < 1) return GM3D_EINVAL;
    if (ncls < 2 || ncls > SVM_MAX_CLS || d > SVM_MAX_D || m > SVM_MAX_N) return GM3D_EUNSUPPORTED;
    if (m == 0) return GM3D_OK;
    if (!X || !w || !rho || !pred || (labels && !correct)) return GM3D_EINVAL;
    return launch_lds<svm_predict_kernel>(dim3((m + PRED_ROWS - 1) / PRED_ROWS), dim3(PRED_THREADS), 0, stream, X, m, d, ncls, w, rho,
                                          labels, pred, reinterpret_cast<unsigned long long*>(correct));
}
