// Small dense complex eigen-algebra on the host and the Krylov-Schur outer iteration built on it: what SLEPc's DS object
// and EPSSolve_KrylovSchur_Default do behind the reference's single call  eps.solve()  (Solver/utils.py:268-270).
//
// Everything here is O(ncv^3) work on the projected (ncv x ncv) matrix; the O(n) parts of the iteration (operator applies,
// orthogonalisation, basis updates) are the device kernels behind lsa_krylov_* (solver.hip).  In tree, no LAPACK: a consumer
// of the C-ABI gets eigenpairs from ONE call (lsa_eigs_sinvert) with nothing but this library loaded, and the result does
// not depend on which BLAS a process happens to carry.
//
//   schur_hessenberg   Householder reduction to Hessenberg form, then the single-shift QR algorithm with Wilkinson shifts,
//                      Schur vectors accumulated (complex arithmetic: the Schur form is upper triangular)
//   schur_swap/reorder adjacent swaps by one rotation each; wanted eigenvalues to the leading block, order kept
//   tri_eigenvectors   back substitution on the triangular factor
//   krylov_schur       Stewart's Krylov-Schur restart: expand to ncv vectors, Schur form with the wanted Ritz values first,
//                      residual estimates |b^H y|, relative convergence test (EPS_CONV_REL), truncate to nconv + (m - nconv)/2
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "lsa_internal.h"

namespace {

struct Z {
    double re, im;
};
inline Z operator+(Z a, Z b) { return {a.re + b.re, a.im + b.im}; }
inline Z operator-(Z a, Z b) { return {a.re - b.re, a.im - b.im}; }
inline Z operator-(Z a) { return {-a.re, -a.im}; }
inline Z operator*(Z a, Z b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
inline Z operator*(double a, Z b) { return {a * b.re, a * b.im}; }
inline Z conj(Z a) { return {a.re, -a.im}; }
inline double abs1(Z a) { return std::fabs(a.re) + std::fabs(a.im); }
inline double abs2(Z a) { return a.re * a.re + a.im * a.im; }
inline double zabs(Z a) { return std::hypot(a.re, a.im); }
inline Z zdiv(Z a, Z b) {  // Smith
    if (std::fabs(b.re) >= std::fabs(b.im)) {
        const double r = b.im / b.re, d = b.re + b.im * r;
        return {(a.re + a.im * r) / d, (a.im - a.re * r) / d};
    }
    const double r = b.re / b.im, d = b.re * r + b.im;
    return {(a.re * r + a.im) / d, (a.im * r - a.re) / d};
}
inline Z zsqrt(Z a) {
    const double m = zabs(a);
    if (m == 0.0) return {0.0, 0.0};
    double re = std::sqrt(0.5 * (m + std::fabs(a.re))), im = 0.5 * a.im / re;
    if (a.re < 0.0) {
        const double t = re;
        re = std::fabs(im);
        im = a.im < 0.0 ? -t : t;
    }
    return {re, im};
}

// rotation R = [c s; -conj(s) c] (c real) with R [f; g] = [r; 0]
inline void givens(Z f, Z g, double& c, Z& s, Z& r) {
    // both entries of ordinary size (LAPACK 3.10's zlartg, unscaled branch): one square root and one division on the chain
    // from one rotation of a QR sweep to the next
    // (squares within (1e-150, 1e150): f2 * h2 <= 2e300 and >= 1e-300 stays a normal number; anything else takes the scaled branch)
    const double f2 = abs2(f), g2 = abs2(g);
    if (f2 > 1e-150 && f2 < 1e150 && g2 > 1e-150 && g2 < 1e150) {
        const double h2 = f2 + g2, d = std::sqrt(f2 * h2), id = 1.0 / d;
        c = f2 * id;
        const Z fd = id * f;
        s = fd * conj(g);
        r = (h2 * id) * f;
        return;
    }
    const double ng = zabs(g);
    if (ng == 0.0) {
        c = 1.0;
        s = {0.0, 0.0};
        r = f;
        return;
    }
    const double nf = zabs(f);
    if (nf == 0.0) {
        c = 0.0;
        s = (1.0 / ng) * conj(g);
        r = {ng, 0.0};
        return;
    }
    const double nrm = std::hypot(nf, ng);
    const Z ph = (1.0 / nf) * f;
    c = nf / nrm;
    s = (1.0 / nrm) * (ph * conj(g));
    r = nrm * ph;
}

// column-major n x n views
struct Mat {
    Z* a;
    int ld;
    inline Z& operator()(int i, int j) const { return a[(size_t)j * ld + i]; }
};

// rows (p, q) of A, columns [j0, j1): [a_p; a_q] <- R [a_p; a_q]
inline void rot_rows(const Mat& A, int p, int q, int j0, int j1, double c, Z s) {
    const Z ms = -conj(s);
    for (int j = j0; j < j1; ++j) {
        const Z x = A(p, j), y = A(q, j);
        A(p, j) = c * x + s * y;
        A(q, j) = ms * x + c * y;
    }
}
// columns (p, q) of A, rows [i0, i1): [a_p a_q] <- [a_p a_q] R^H
inline void rot_cols(const Mat& A, int p, int q, int i0, int i1, double c, Z s) {
    Z* xp = &A(0, p);
    Z* xq = &A(0, q);
    const Z cs = conj(s);
    for (int i = i0; i < i1; ++i) {
        const Z x = xp[i], y = xq[i];
        xp[i] = c * x + cs * y;
        xq[i] = c * y - s * x;
    }
}

// A <- P^H A P (upper Hessenberg on return), Q <- Q P;  Q must hold a unitary matrix on entry (the identity, or a basis to carry along).
// Row-oriented, from the bottom: row r keeps only its entry in column r - 1 of those left of the diagonal, by a Householder
// reflector on the coordinates 0 .. r - 1.  Rows that conform already cost nothing, so the matrix of a Krylov-Schur restart
// (triangle of k rows, one full row, Hessenberg below) costs the reduction of a k x k matrix, not of the whole.
__attribute__((always_inline)) inline void hessenberg_reduce_body(int n, const Mat& A, const Mat& Q) {
    std::vector<Z> v((size_t)n), w((size_t)n);
    for (int r = n - 1; r >= 2; --r) {
        // x = A[r, 0:r]: wanted x^T P = gamma e_{r-1}^T with P = I - tp v v^H on the coordinates 0 .. r - 1
        double xnorm2 = 0.0;
        for (int j = 0; j < r - 1; ++j) xnorm2 += abs2(A(r, j));
        if (xnorm2 == 0.0) continue;
        const Z alpha = A(r, r - 1);
        const double nrm = std::sqrt(abs2(alpha) + xnorm2);
        const double beta = alpha.re >= 0.0 ? -nrm : nrm;
        // LAPACK's zlarfg on (alpha; x): G^H (alpha; x) = beta e, G = I - tau u u^H, u = (1; x / (alpha - beta)).  Here P^T = G^H,
        // i.e. v = conj(u) and tp = conj(tau).
        const Z tau = {(beta - alpha.re) / beta, -alpha.im / beta};
        const Z scale = zdiv({1.0, 0.0}, alpha - Z{beta, 0.0});
        const Z tp = conj(tau);
        v[(size_t)r - 1] = {1.0, 0.0};
        for (int j = 0; j < r - 1; ++j) v[(size_t)j] = conj(scale * A(r, j));
        // right: B[0:r+1, 0:r] -= tp (B v) v^H  (rows below r have no entries in these columns), and Q[:, 0:r] likewise
        for (int pass = 0; pass < 2; ++pass) {
            const Mat& B = pass == 0 ? A : Q;
            const int rows = pass == 0 ? r + 1 : n;
            for (int i = 0; i < rows; ++i) w[(size_t)i] = {0.0, 0.0};
            for (int j = 0; j < r; ++j) {
                const Z vj = v[(size_t)j];
                const Z* col = &B(0, j);
                for (int i = 0; i < rows; ++i) w[(size_t)i] = w[(size_t)i] + col[i] * vj;
            }
            for (int j = 0; j < r; ++j) {
                const Z f = tp * conj(v[(size_t)j]);
                Z* col = &B(0, j);
                for (int i = 0; i < rows; ++i) col[i] = col[i] - w[(size_t)i] * f;
            }
        }
        A(r, r - 1) = {beta, 0.0};
        for (int j = 0; j < r - 1; ++j) A(r, j) = {0.0, 0.0};
        // left: A[0:r, :] -= conj(tp) v (v^H A[0:r, :])
        const Z ctp = conj(tp);
        for (int j = 0; j < n; ++j) {
            Z d = {0.0, 0.0};
            Z* col = &A(0, j);
            for (int i = 0; i < r; ++i) d = d + conj(v[(size_t)i]) * col[i];
            d = ctp * d;
            for (int i = 0; i < r; ++i) col[i] = col[i] - v[(size_t)i] * d;
        }
    }
}
// the same body built for the host's vector width (the loops are complex axpys and dot products down contiguous columns)
void hessenberg_reduce_generic(int n, const Mat& A, const Mat& Q) { hessenberg_reduce_body(n, A, Q); }
#if !defined(__HIP_DEVICE_COMPILE__)
__attribute__((target("avx2,fma"))) void hessenberg_reduce_avx2(int n, const Mat& A, const Mat& Q) { hessenberg_reduce_body(n, A, Q); }
__attribute__((target("avx512f,avx512dq,fma"), min_vector_width(512))) void hessenberg_reduce_avx512(int n, const Mat& A, const Mat& Q) {
    hessenberg_reduce_body(n, A, Q);
}
#endif
void hessenberg_reduce(int n, const Mat& A, const Mat& Q) {
#if !defined(__HIP_DEVICE_COMPILE__)
    __builtin_cpu_init();
    static const char* isa = getenv("LSA_DENSE_ISA");
    static const bool want512 = !isa || !strcmp(isa, "avx512"), want256 = want512 || !strcmp(isa, "avx2");
    static const int level = (want512 && __builtin_cpu_supports("avx512f") && __builtin_cpu_supports("avx512dq") && __builtin_cpu_supports("fma")) ? 2
                             : (want256 && __builtin_cpu_supports("avx2") && __builtin_cpu_supports("fma"))                                     ? 1
                                                                                                                                                 : 0;
    if (level == 2) return hessenberg_reduce_avx512(n, A, Q);
    if (level == 1) return hessenberg_reduce_avx2(n, A, Q);
#endif
    hessenberg_reduce_generic(n, A, Q);
}

// [x; y] <- R [x; y] element-wise on split (real / imaginary) contiguous arrays: the inner loops of the QR sweeps.
// R = [c s; -conj(s) c].  The arrays start on 64-byte lines and `len` is a multiple of 8 (rows and columns of the work
// layout are padded to that).  Two builds of the same body: the portable one and one for AVX2 + FMA hosts, picked at run time.
#define LSA_ROT_BODY                                                     \
    xr = (double*)__builtin_assume_aligned(xr, 64);                      \
    xi = (double*)__builtin_assume_aligned(xi, 64);                      \
    yr = (double*)__builtin_assume_aligned(yr, 64);                      \
    yi = (double*)__builtin_assume_aligned(yi, 64);                      \
    len &= ~7; /* callers pass whole 64-byte lines: no peeled head, no scalar tail */ \
    for (int j = 0; j < len; ++j) {                                      \
        const double ar = xr[j], ai = xi[j], br = yr[j], bi = yi[j];     \
        xr[j] = c * ar + (sr * br - si * bi);                            \
        xi[j] = c * ai + (sr * bi + si * br);                            \
        yr[j] = c * br - (sr * ar + si * ai);                            \
        yi[j] = c * bi - (sr * ai - si * ar);                            \
    }
void rot_pair_generic(int len, double* __restrict__ xr, double* __restrict__ xi, double* __restrict__ yr, double* __restrict__ yi, double c, double sr,
                      double si) {
    LSA_ROT_BODY
}
#if !defined(__HIP_DEVICE_COMPILE__)  // (this file is host code; the device pass of the compiler knows neither the target nor the builtins)
__attribute__((target("avx2,fma"))) void rot_pair_avx2(int len, double* __restrict__ xr, double* __restrict__ xi, double* __restrict__ yr,
                                                       double* __restrict__ yi, double c, double sr, double si) {
    LSA_ROT_BODY
}
__attribute__((target("avx512f,avx512dq,fma"), min_vector_width(512))) void rot_pair_avx512(int len, double* __restrict__ xr, double* __restrict__ xi,
                                                                                             double* __restrict__ yr, double* __restrict__ yi, double c,
                                                                                             double sr, double si) {
    LSA_ROT_BODY
}
#endif
#undef LSA_ROT_BODY
typedef void (*rot_pair_fn)(int, double*, double*, double*, double*, double, double, double);

// columns k, k + 1 of one row of the split planes (pr, pi point at column k): [a b] <- [a b] R^H, R^H = [c -s; conj(s) c], i.e.
// a' = c a + conj(s) b, b' = c b - s a.  The two columns are neighbours in memory: one 16-byte vector per plane, with
// cc = {c, c}, srn = {Re s, -Re s}, sii = {Im s, Im s}.
typedef double v2d __attribute__((ext_vector_type(2)));
inline void rot_cols2(double* pr, double* pi, v2d cc, v2d srn, v2d sii) {
    v2d vr, vi;
    memcpy(&vr, pr, sizeof vr);
    memcpy(&vi, pi, sizeof vi);
    const v2d wr = __builtin_shufflevector(vr, vr, 1, 0), wi = __builtin_shufflevector(vi, vi, 1, 0);
    const v2d nr = cc * vr + (srn * wr + sii * wi);
    const v2d ni = cc * vi + (srn * wi - sii * wr);
    memcpy(pr, &nr, sizeof nr);
    memcpy(pi, &ni, sizeof ni);
}
rot_pair_fn pick_rot_pair() {
#if !defined(__HIP_DEVICE_COMPILE__)
    __builtin_cpu_init();
    const char* isa = getenv("LSA_DENSE_ISA");  // "avx2" / "generic": measurement aid
    const bool want512 = !isa || !strcmp(isa, "avx512"), want256 = want512 || !strcmp(isa, "avx2");
    if (want512 && __builtin_cpu_supports("avx512f") && __builtin_cpu_supports("avx512dq") && __builtin_cpu_supports("fma")) return rot_pair_avx512;
    if (want256 && __builtin_cpu_supports("avx2") && __builtin_cpu_supports("fma")) return rot_pair_avx2;
#endif
    return rot_pair_generic;
}

// Schur form of an upper Hessenberg H (in place: upper triangular T on return), Q <- Q U with H = U T U^H.
// Single-shift QR with Wilkinson shifts and the standard small-subdiagonal deflation test; returns false if an eigenvalue
// fails to converge in 30 sweeps per eigenvalue (does not happen for the Rayleigh quotients of an Arnoldi process).
//
// Work layout (80 x 80 is 2.9 ms with complex scalars in column-major storage, four times per 30 k-unknown eigen-solve, the GPU
// idle meanwhile): H is kept ROW-major and Q column-major, both split into real and imaginary planes, so that the two long
// updates of every rotation -- rows k, k + 1 of H to the right of the bulge, columns k, k + 1 of Q -- are contiguous real
// loops the compiler vectorises.  The column update of H inside the active window (a few rows around the bulge) stays
// strided; its part ABOVE the window (rows that only collect the sweep's rotations) is applied after the sweep, row by row,
// four rows at a time.
bool hessenberg_qr(int n, const Mat& H, const Mat& Q) {
    static const rot_pair_fn rot_pair = pick_rot_pair();
    const double ulp = 2.220446049250313e-16, smlnum = 2.2250738585072014e-308 * (n / ulp);
    const int ld = (n + 7) & ~7;  // whole 64-byte lines per row of H / column of Q; the padding holds zeros and stays zero
    std::vector<double> store((size_t)4 * ld * std::max(n, 1) + 8, 0.0);
    double* hr = (double*)(((uintptr_t)store.data() + 63) & ~(uintptr_t)63);  // hr[i * ld + j] = Re H(i, j)
    double* hi = hr + (size_t)ld * n;
    double* qr = hi + (size_t)ld * n;     // qr[j * ld + i] = Re Q(i, j)
    double* qi = qr + (size_t)ld * n;
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i) {
            hr[(size_t)i * ld + j] = H(i, j).re;
            hi[(size_t)i * ld + j] = H(i, j).im;
            qr[(size_t)j * ld + i] = Q(i, j).re;
            qi[(size_t)j * ld + i] = Q(i, j).im;
        }
    auto h = [&](int i, int j) { return Z{hr[(size_t)i * ld + j], hi[(size_t)i * ld + j]}; };
    auto seth = [&](int i, int j, Z v) {
        hr[(size_t)i * ld + j] = v.re;
        hi[(size_t)i * ld + j] = v.im;
    };
    std::vector<double> rc((size_t)n), rsr((size_t)n), rsi((size_t)n);  // the rotations of the current sweep
    int ihi = n - 1;
    int its = 0, total = 0;
    bool ok = true;
    while (ihi >= 0) {
        int l = ihi;
        for (; l > 0; --l) {
            const double sub = abs1(h(l, l - 1));
            if (sub <= smlnum) break;
            double tst = abs1(h(l - 1, l - 1)) + abs1(h(l, l));
            if (tst == 0.0) {
                if (l - 2 >= 0) tst += abs1(h(l - 1, l - 2));
                if (l + 1 <= ihi) tst += abs1(h(l + 1, l));
            }
            if (sub <= ulp * tst) {
                // (Ahues & Tisseur) a small subdiagonal next to diagonal entries of very different size
                const double ab = std::max(abs1(h(l, l - 1)), abs1(h(l - 1, l))), ba = std::min(abs1(h(l, l - 1)), abs1(h(l - 1, l)));
                const Z dd = h(l - 1, l - 1) - h(l, l);
                const double aa = std::max(abs1(h(l, l)), abs1(dd)), bb = std::min(abs1(h(l, l)), abs1(dd));
                const double s = aa + ab;
                if (ba * (ab / s) <= std::max(smlnum, ulp * (bb * (aa / s)))) break;
            }
        }
        if (l > 0) seth(l, l - 1, {0.0, 0.0});
        if (l == ihi) {  // one eigenvalue has split off
            --ihi;
            its = 0;
            continue;
        }
        // (LAPACK's zlahqr allows 30 * max(10, n) sweeps per eigenvalue with an exceptional shift every tenth; giving up after 30
        //  aborted whole eigen-solves on clustered projected matrices.  The subdiagonals are not kept real here: abs1, not .re)
        if (++its > 30 * std::max(10, n) || ++total > 30 * std::max(10, n) * n) {
            ok = false;
            break;
        }
        Z shift;
        if (its % 20 == 10) {
            shift = h(l, l) + Z{0.75 * abs1(h(l + 1, l)), 0.0};
        } else if (its % 20 == 0) {
            shift = h(ihi, ihi) + Z{0.75 * abs1(h(ihi, ihi - 1)), 0.0};
        } else {
            // the eigenvalue of the trailing 2 x 2 block nearer to its last diagonal entry
            shift = h(ihi, ihi);
            const Z u2 = h(ihi - 1, ihi) * h(ihi, ihi - 1);
            if (abs1(u2) != 0.0) {
                const Z x = 0.5 * (h(ihi - 1, ihi - 1) - shift);
                const Z y = zsqrt(x * x + u2);
                const Z d = x.re * y.re + x.im * y.im < 0.0 ? x - y : x + y;  // the larger of x +- y
                shift = shift - zdiv(u2, d);
            }
        }
        // one implicit single-shift sweep over rows l .. ihi
        Z x = h(l, l) - shift, y = h(l + 1, l);
        for (int k = l; k < ihi; ++k) {
            double c;
            Z s, r;
            givens(x, y, c, s, r);
            rc[(size_t)k] = c;
            rsr[(size_t)k] = s.re;
            rsi[(size_t)k] = s.im;
            // rows k, k + 1 <- R rows, from the 64-byte line that holds column k to the end of the padded row (contiguous whole
            // vectors; left of column k - 1 both rows hold zeros, and column k - 1 -- the bulge -- gets its exact values below)
            const int k0 = k & ~7;
            rot_pair(ld - k0, hr + (size_t)k * ld + k0, hi + (size_t)k * ld + k0, hr + (size_t)(k + 1) * ld + k0, hi + (size_t)(k + 1) * ld + k0, c, s.re, s.im);
            if (k > l) {
                seth(k, k - 1, r);
                seth(k + 1, k - 1, {0.0, 0.0});
            }
            // columns k, k + 1 <- columns R^H, rows l .. min(k + 2, ihi) (the window; strided).  With R^H = [c -s; conj(s) c]:
            // new_k = c a + conj(s) b,  new_k1 = c b - s a
            const int i1 = std::min(k + 2, ihi);
            const v2d cc = {c, c}, srn = {s.re, -s.re}, sii = {s.im, s.im};
            for (int i = l; i <= i1; ++i) rot_cols2(hr + (size_t)i * ld + k, hi + (size_t)i * ld + k, cc, srn, sii);
            // columns k, k + 1 of Q <- columns R^H (contiguous): in the form of rot_pair, [x; y] <- [c conj(s); -s c] [x; y],
            // i.e. the rotation with s replaced by conj(s).  (Tried: Q's rotations of a whole sweep after the sweep, eight rows at
            // a time with column k carried in registers -- half the loads and stores, and slower: 2.16-2.28 against 1.99-2.06 ms.)
            rot_pair(ld, qr + (size_t)k * ld, qi + (size_t)k * ld, qr + (size_t)(k + 1) * ld, qi + (size_t)(k + 1) * ld, c, s.re, -s.im);
            if (k + 1 < ihi) {
                x = h(k + 1, k);
                y = h(k + 2, k);
            }
        }
        // the rows above the window collect the sweep's column rotations, one row after the other (four rows interleaved)
        for (int i0 = 0; i0 < l; i0 += 4) {
            const int ni = std::min(4, l - i0);
            for (int k = l; k < ihi; ++k) {
                const v2d cc = {rc[(size_t)k], rc[(size_t)k]}, srn = {rsr[(size_t)k], -rsr[(size_t)k]}, sii = {rsi[(size_t)k], rsi[(size_t)k]};
                for (int u = 0; u < ni; ++u) rot_cols2(hr + (size_t)(i0 + u) * ld + k, hi + (size_t)(i0 + u) * ld + k, cc, srn, sii);
            }
        }
    }
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i) {
            H(i, j) = (ok && i > j) ? Z{0.0, 0.0} : Z{hr[(size_t)i * ld + j], hi[(size_t)i * ld + j]};
            Q(i, j) = {qr[(size_t)j * ld + i], qi[(size_t)j * ld + i]};
        }
    return ok;
}

// T, Q: Schur form.  Swaps the diagonal entries k and k + 1 by one rotation (LAPACK's ztrexc step).
void schur_swap(int n, const Mat& T, const Mat& Q, int k) {
    const Z t11 = T(k, k), t22 = T(k + 1, k + 1);
    double c;
    Z s, r;
    givens(T(k, k + 1), t22 - t11, c, s, r);
    if (k + 2 < n) rot_rows(T, k, k + 1, k + 2, n, c, s);
    rot_cols(T, k, k + 1, 0, k, c, s);
    T(k, k) = t22;
    T(k + 1, k + 1) = t11;
    rot_cols(Q, k, k + 1, 0, n, c, s);
}

// moves the selected diagonal entries to the leading block (their relative order and that of the others kept); returns their count
int schur_reorder(int n, const Mat& T, const Mat& Q, const std::vector<char>& select) {
    int ks = 0;
    for (int k = 0; k < n; ++k) {
        if (!select[(size_t)k]) continue;
        for (int i = k; i > ks; --i) schur_swap(n, T, Q, i - 1);
        ++ks;
    }
    return ks;
}

// right eigenvectors of the upper triangular T: S[:, k], unit 2-norm
void tri_eigenvectors(int n, const Mat& T, const Mat& S) {
    const double ulp = 2.220446049250313e-16, smlnum = 2.2250738585072014e-308 * (n / ulp);
    double tnorm = 0.0;
    for (int j = 0; j < n; ++j)
        for (int i = 0; i <= j; ++i) tnorm = std::max(tnorm, abs1(T(i, j)));
    for (int k = 0; k < n; ++k) {
        const Z lam = T(k, k);
        const double smin = std::max(ulp * std::max(abs1(lam), tnorm * 1e-3), smlnum);
        for (int i = k + 1; i < n; ++i) S(i, k) = {0.0, 0.0};
        S(k, k) = {1.0, 0.0};
        for (int i = 0; i < k; ++i) S(i, k) = -T(i, k);
        for (int i = k - 1; i >= 0; --i) {
            Z d = T(i, i) - lam;
            if (abs1(d) < smin) d = {smin, 0.0};
            const Z xi = zdiv(S(i, k), d);
            S(i, k) = xi;
            if (abs1(xi) > 1e150) {  // (never met on Rayleigh quotients; keeps the substitution finite)
                for (int q = 0; q <= k; ++q) S(q, k) = 1e-150 * S(q, k);
            }
            const Z xs = S(i, k);
            for (int q = 0; q < i; ++q) S(q, k) = S(q, k) - T(q, i) * xs;
        }
        double nrm = 0.0;
        for (int i = 0; i <= k; ++i) nrm += abs2(S(i, k));
        nrm = 1.0 / std::sqrt(nrm);
        for (int i = 0; i <= k; ++i) S(i, k) = nrm * S(i, k);
    }
}

bool is_hessenberg(int n, const Mat& A) {
    for (int j = 0; j + 2 < n; ++j)
        for (int i = j + 2; i < n; ++i)
            if (A(i, j).re != 0.0 || A(i, j).im != 0.0) return false;
    return true;
}

// complex Schur form of a general square matrix: A = Q T Q^H, T over A, Q written
bool schur(int n, const Mat& A, const Mat& Q) {
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i) Q(i, j) = {i == j ? 1.0 : 0.0, 0.0};
    if (!is_hessenberg(n, A)) hessenberg_reduce(n, A, Q);
    return hessenberg_qr(n, A, Q);
}

// ---- eigenvalue selection (SLEPc's EPSWhich on lambda, Solver/utils.py:152-187 of the reference) -------------------------------
struct Selector {
    int which, transform;
    Z sigma, nu, target;
    Z back(Z th) const {  // Ritz value of the transformed operator -> eigenvalue of the pencil
        const double tiny = 2.2250738585072014e-308;
        if (transform == 0) {  // shift-invert: theta = 1 / (lambda - sigma)
            if (th.re == 0.0 && th.im == 0.0) th = {tiny, 0.0};
            return sigma + zdiv({1.0, 0.0}, th);
        }
        if (transform == 2) {  // Cayley: theta = (lambda + nu) / (lambda - sigma)
            Z d = th - Z{1.0, 0.0};
            if (th.re == 1.0 && th.im == 0.0) d = {1e-300, 0.0};
            return zdiv(sigma * th + nu, d);
        }
        return th + sigma;  // shift
    }
    double key(Z th) const {  // small = wanted
        const Z lam = back(th);
        switch (which) {
            case LSA_WHICH_LARGEST_MAGNITUDE: return -zabs(lam);
            case LSA_WHICH_LARGEST_REAL: return -lam.re;
            case LSA_WHICH_SMALLEST_REAL: return lam.re;
            case LSA_WHICH_LARGEST_IMAGINARY: return -lam.im;
            case LSA_WHICH_SMALLEST_IMAGINARY: return lam.im;
            case LSA_WHICH_TARGET_REAL: return std::fabs(lam.re - target.re);
            case LSA_WHICH_TARGET_IMAGINARY: return std::fabs(lam.im - target.im);
            default: return zabs(lam - target);  // LSA_WHICH_TARGET_MAGNITUDE
        }
    }
};

inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct Rng {  // splitmix64 + Box-Muller: start vectors and the fresh directions after a breakdown
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    double uniform() { return ((next() >> 11) + 0.5) * (1.0 / 9007199254740992.0); }
    void normal_pair(double& a, double& b) {
        const double r = std::sqrt(-2.0 * std::log(uniform())), t = 6.283185307179586 * uniform();
        a = r * std::cos(t);
        b = r * std::sin(t);
    }
};

// ---- real symmetric eigenproblem (the projected matrix of the Lanczos iteration) ---------------------------------------------
// Householder reduction to tridiagonal form with the transformations accumulated, then the implicit QL algorithm with Wilkinson
// shifts (EISPACK's tred2 / tql2, Wilkinson & Reinsch, Handbook for Automatic Computation II).  a: n x n column-major with leading
// dimension lda, lower triangle read, eigenvectors written over it; d: eigenvalues ascending.  The matrix is scaled by a power of
// two to max|a| ~ 1 first, so that the sums of squares neither overflow nor underflow.  false: the QL iteration stalled.
bool sym_eig(int n, double* a, int lda, double* d) {
    if (n == 0) return true;
    auto A = [&](int i, int j) -> double& { return a[(size_t)j * lda + i]; };
    double amax = 0.0;
    for (int j = 0; j < n; ++j)
        for (int i = j; i < n; ++i) {
            if (!std::isfinite(A(i, j))) return false;
            amax = std::max(amax, std::fabs(A(i, j)));
        }
    if (amax == 0.0) {
        for (int j = 0; j < n; ++j) {
            for (int i = 0; i < n; ++i) A(i, j) = i == j ? 1.0 : 0.0;
            d[j] = 0.0;
        }
        return true;
    }
    int ex = 0;
    (void)std::frexp(amax, &ex);
    const double scale = std::ldexp(1.0, -ex), unscale = std::ldexp(1.0, ex);
    for (int j = 0; j < n; ++j)
        for (int i = j; i < n; ++i) {
            const double v = A(i, j) * scale;
            A(i, j) = v;
            A(j, i) = v;
        }
    std::vector<double> e((size_t)n, 0.0);
    // -- tred2
    for (int j = 0; j < n; ++j) d[j] = A(n - 1, j);
    for (int i = n - 1; i > 0; --i) {
        double sc = 0.0, h = 0.0;
        for (int k = 0; k < i; ++k) sc += std::fabs(d[k]);
        if (sc == 0.0) {
            e[i] = d[i - 1];
            for (int j = 0; j < i; ++j) {
                d[j] = A(i - 1, j);
                A(i, j) = 0.0;
                A(j, i) = 0.0;
            }
        } else {
            for (int k = 0; k < i; ++k) {
                d[k] /= sc;
                h += d[k] * d[k];
            }
            double f = d[i - 1], g = std::sqrt(h);
            if (f > 0.0) g = -g;
            e[i] = sc * g;
            h -= f * g;
            d[i - 1] = f - g;
            for (int j = 0; j < i; ++j) e[j] = 0.0;
            for (int j = 0; j < i; ++j) {
                f = d[j];
                A(j, i) = f;
                g = e[j] + A(j, j) * f;
                for (int k = j + 1; k <= i - 1; ++k) {
                    g += A(k, j) * d[k];
                    e[k] += A(k, j) * f;
                }
                e[j] = g;
            }
            f = 0.0;
            for (int j = 0; j < i; ++j) {
                e[j] /= h;
                f += e[j] * d[j];
            }
            const double hh = f / (h + h);
            for (int j = 0; j < i; ++j) e[j] -= hh * d[j];
            for (int j = 0; j < i; ++j) {
                f = d[j];
                g = e[j];
                for (int k = j; k <= i - 1; ++k) A(k, j) -= f * e[k] + g * d[k];
                d[j] = A(i - 1, j);
                A(i, j) = 0.0;
            }
        }
        d[i] = h;
    }
    for (int i = 0; i < n - 1; ++i) {
        A(n - 1, i) = A(i, i);
        A(i, i) = 1.0;
        const double h = d[i + 1];
        if (h != 0.0) {
            for (int k = 0; k <= i; ++k) d[k] = A(k, i + 1) / h;
            for (int j = 0; j <= i; ++j) {
                double g = 0.0;
                for (int k = 0; k <= i; ++k) g += A(k, i + 1) * A(k, j);
                for (int k = 0; k <= i; ++k) A(k, j) -= g * d[k];
            }
        }
        for (int k = 0; k <= i; ++k) A(k, i + 1) = 0.0;
    }
    for (int j = 0; j < n; ++j) {
        d[j] = A(n - 1, j);
        A(n - 1, j) = 0.0;
    }
    A(n - 1, n - 1) = 1.0;
    e[0] = 0.0;
    // -- tql2
    for (int i = 1; i < n; ++i) e[i - 1] = e[i];
    e[n - 1] = 0.0;
    double f = 0.0, tst1 = 0.0;
    const double eps = 2.220446049250313e-16;
    for (int l = 0; l < n; ++l) {
        tst1 = std::max(tst1, std::fabs(d[l]) + std::fabs(e[l]));
        int m = l;
        while (m < n - 1) {
            if (std::fabs(e[m]) <= eps * tst1) break;
            ++m;
        }
        if (m > l) {
            int iter = 0;
            do {
                if (++iter > 60) return false;
                double g = d[l];
                double p = (d[l + 1] - g) / (2.0 * e[l]);
                double r = std::hypot(p, 1.0);
                if (p < 0.0) r = -r;
                d[l] = e[l] / (p + r);
                d[l + 1] = e[l] * (p + r);
                const double dl1 = d[l + 1];
                double h = g - d[l];
                for (int i = l + 2; i < n; ++i) d[i] -= h;
                f += h;
                p = d[m];
                double c = 1.0, c2 = c, c3 = c, s = 0.0, s2 = 0.0;
                const double el1 = e[l + 1];
                for (int i = m - 1; i >= l; --i) {
                    c3 = c2;
                    c2 = c;
                    s2 = s;
                    g = c * e[i];
                    h = c * p;
                    r = std::hypot(p, e[i]);
                    e[i + 1] = s * r;
                    s = e[i] / r;
                    c = p / r;
                    p = c * d[i] - s * g;
                    d[i + 1] = h + s * (c * g + s * d[i]);
                    for (int k = 0; k < n; ++k) {
                        h = A(k, i + 1);
                        A(k, i + 1) = s * A(k, i) + c * h;
                        A(k, i) = c * A(k, i) - s * h;
                    }
                }
                p = -s * s2 * c3 * el1 * e[l] / dl1;
                e[l] = s * p;
                d[l] = c * p;
            } while (std::fabs(e[l]) > eps * tst1);
        }
        d[l] += f;
        e[l] = 0.0;
    }
    // ascending order (selection sort: the columns move with their values)
    for (int i = 0; i < n - 1; ++i) {
        int k = i;
        double p = d[i];
        for (int j = i + 1; j < n; ++j)
            if (d[j] < p) k = j, p = d[j];
        if (k != i) {
            d[k] = d[i];
            d[i] = p;
            for (int j = 0; j < n; ++j) std::swap(A(j, i), A(j, k));
        }
    }
    for (int j = 0; j < n; ++j) d[j] *= unscale;
    return true;
}

// ---- what the two outer loops (lsa_krylov_solve, lsa_lanczos_solve) share ------------------------------------------------
int ks_check_options(lsa_ctx* ctx, const char* who, const lsa_ks_options* o, int32_t max_out, const void* theta_out, const void* lambda_out) {
    if (o->nev < 1 || o->max_restarts < 0 || !(o->tol > 0.0) || max_out < 0 || (max_out > 0 && (!theta_out || !lambda_out)))
        return lsa_set_error(ctx, LSA_ERR_ARG, "%s: nev, tol must be positive, output buffers are required", who);
    return LSA_OK;
}
double ks_keep_fraction(const lsa_ks_options* o) { return o->keep_fraction > 0.0 && o->keep_fraction < 1.0 ? o->keep_fraction : 0.5; }
Rng ks_rng(const lsa_ks_options* o) { return Rng{o->seed * 0x2545F4914F6CDD1Dull + 0x1234567ull}; }

// Expand the basis from `kept` to m vectors; continue past exact breakdowns (invariant subspace) with a fresh direction.
// extend(j, &bd): the steps [j, m), bd = the step that broke down or -1; inject_random(j): a random vector orthonormalised into
// column j.  Adds the operator applies to *applies.
template <class Extend, class InjectRandom>
int ks_expand(int kept, int m, int64_t* applies, Extend extend, InjectRandom inject_random) {
    int j = kept;
    while (j < m) {
        int32_t bd = -1;
        LSA_CHECK(extend(j, &bd));
        if (bd < 0) {
            *applies += m - j;
            break;
        }
        *applies += bd - j + 1;
        if (bd + 1 >= m) break;  // broke down on the last step: the m vectors span an invariant subspace
        LSA_CHECK(inject_random(bd + 1));
        j = bd + 1;
    }
    return LSA_OK;
}

// rank <- 0..m-1 sorted by key (stable); returns how many of the leading ones have a relative residual estimate within tol
int ks_rank_converged(int m, const std::vector<double>& keys, const std::vector<double>& rel, double tol, std::vector<int>& rank) {
    for (int c = 0; c < m; ++c) rank[(size_t)c] = c;
    std::stable_sort(rank.begin(), rank.end(), [&](int x, int y) { return keys[(size_t)x] < keys[(size_t)y]; });
    int nconv = 0;
    while (nconv < m && rel[(size_t)rank[(size_t)nconv]] <= tol) ++nconv;
    return nconv;
}

// vectors kept by a restart: the converged ones and keep_fraction of the rest, at least one and at most m - 1
int ks_keep_count(int m, int nconv, double keep_fraction) { return std::max(std::min(nconv + (int)((m - nconv) * keep_fraction), m - 1), 1); }

struct KsClock {  // seconds per phase of the outer loop; lap() books the time since the last lap
    double expand = 0.0, dense = 0.0, restart = 0.0, t0 = 0.0;
    void start() { t0 = now_s(); }
    void lap(double& phase) {
        const double t = now_s();
        phase += t - t0;
        t0 = t;
    }
};

void ks_fill_result(lsa_ks_result* r, const KsClock& clk, int nconv, int nout, int restarts, int64_t applies, double next_unconverged) {
    r->seconds_expand = clk.expand;
    r->seconds_dense = clk.dense;
    r->seconds_restart = clk.restart;
    r->nconv = nconv;
    r->nout = nout;
    r->restarts = restarts;
    r->op_applies = applies;
    r->next_unconverged = next_unconverged;
}

// ---- the thick-restart Lanczos loop, once, for the three bases it serves ----------------------------------------------------------
// The real M-orthonormal basis of a symmetric-definite pencil (lanczos.hip), the complex one of the resolvent's W (resolvent.hip) and
// the real one of the transient-growth W (growth.hip) have one and the same real symmetric projected matrix; the loop reaches a basis through extend, inject, restart and vectors, and
// ranks and maps the Ritz values through key and back.
struct TrlRealBasis {
    using scalar = double;
    lsa_ctx* ctx;
    lsa_lanczos* l;
    Selector sel;
    int64_t n = 0;
    int32_t m = 0;
    void random(Rng& rng, std::vector<double>& vec) const {
        double other = 0.0;
        for (int64_t i = 0; i < n; ++i) rng.normal_pair(vec[(size_t)i], other);
    }
    int inject(int j, const double* v) { return lanczos_inject(ctx, l, j, v); }
    int extend(int j, double* T, int ldt, int32_t* bd) { return lsa_lanczos_extend(ctx, l, j, m, T, ldt, bd); }
    int restart(int knew, const double* Yk) { return lanczos_restart(ctx, l, m, knew, Yk, m); }
    int vectors(int nout, const double* Yo, const double*, double* X) { return lanczos_ritz_vectors(ctx, l, m, nout, Yo, m, X); }
    double key(double theta) const { return sel.key(Z{theta, 0.0}); }
    double back(double theta) const { return sel.back(Z{theta, 0.0}).re; }
};

struct TrlResolventBasis {
    using scalar = cplx;
    lsa_ctx* ctx;
    lsa_resolvent* r;
    cplx* F;  // the forcings' destination, or null
    int64_t n = 0;
    int32_t m = 0;
    void random(Rng& rng, std::vector<cplx>& vec) const {
        for (int64_t i = 0; i < n; ++i) rng.normal_pair(vec[(size_t)i].re, vec[(size_t)i].im);
    }
    int inject(int j, const cplx* v) { return resolvent_inject(ctx, r, j, v); }
    int extend(int j, double* T, int ldt, int32_t* bd) { return lsa_resolvent_extend(ctx, r, j, m, T, ldt, bd); }
    int restart(int knew, const double* Yk) { return resolvent_restart(ctx, r, m, knew, Yk, m); }
    int vectors(int nout, const double* Yo, const double* gains, cplx* Q) {
        LSA_CHECK(resolvent_ritz_vectors(ctx, r, m, nout, Yo, m, Q));
        return F ? resolvent_forcings(ctx, r, nout, gains, F) : LSA_OK;
    }
    double key(double theta) const { return -theta; }  // the largest gains first
    double back(double theta) const { return theta > 0.0 ? std::sqrt(theta) : 0.0; }  // theta = sigma^2
};

struct TrlGrowthBasis {
    using scalar = double;
    lsa_ctx* ctx;
    lsa_growth* g;
    double *QT, *energy;  // the responses' and the energy curves' destinations, or null
    int64_t n = 0;
    int32_t m = 0;
    void random(Rng& rng, std::vector<double>& vec) const {
        double other = 0.0;
        for (int64_t i = 0; i < n; ++i) rng.normal_pair(vec[(size_t)i], other);
    }
    int inject(int j, const double* v) { return growth_inject(ctx, g, j, v); }
    int extend(int j, double* T, int ldt, int32_t* bd) { return lsa_growth_extend(ctx, g, j, m, T, ldt, bd); }
    int restart(int knew, const double* Yk) { return growth_restart(ctx, g, m, knew, Yk, m); }
    int vectors(int nout, const double* Yo, const double*, double* Q0) {
        LSA_CHECK(growth_ritz_vectors(ctx, g, m, nout, Yo, m, Q0));
        return (QT || energy) ? growth_responses(ctx, g, nout, QT, energy) : LSA_OK;
    }
    double key(double theta) const { return -theta; }  // the largest gains first
    double back(double theta) const { return theta; }   // theta = G itself
};

struct TrlStochasticBasis {
    using scalar = double;
    lsa_ctx* ctx;
    lsa_stochastic* h;
    int64_t n = 0;
    int32_t m = 0;
    void random(Rng& rng, std::vector<double>& vec) const {
        double other = 0.0;
        for (int64_t i = 0; i < n; ++i) rng.normal_pair(vec[(size_t)i], other);
    }
    int inject(int j, const double* v) { return stochastic_inject(ctx, h, j, v); }
    int extend(int j, double* T, int ldt, int32_t* bd) { return stochastic_extend(ctx, h, j, m, T, ldt, bd); }
    int restart(int knew, const double* Yk) { return stochastic_restart(ctx, h, m, knew, Yk, m); }
    int vectors(int nout, const double* Yo, const double*, double* X) { return stochastic_ritz_vectors(ctx, h, m, nout, Yo, m, X); }
    double key(double theta) const { return -theta; }  // the largest variances first
    double back(double theta) const { return theta; }
};

// What the loop keeps per problem: the projected matrix, its eigenvectors, the vectors kept, the counters, the clock, the generator and
// the result, as KsState does for Krylov-Schur.  trl_solve is the loop over one state; lsa_resolvent_solve_batch the loop over J.
template <class Basis>
struct TrlState {
    using S = typename Basis::scalar;
    lsa_ctx* ctx;
    Basis b;
    const lsa_ks_options* o;
    int32_t max_out;
    double *theta_out, *lambda_out;
    S* X_out;
    double* est_out;
    lsa_ks_result* result;
    int32_t m = 0;
    int64_t n = 0;
    int nev = 0, ldt = 0;
    double keep_fraction = 0.5;
    Rng rng;
    std::vector<S> vec;
    std::vector<double> T, Y, theta, est, rel, keys;
    std::vector<int> rank;
    int kept = 0, restarts = 0;
    int64_t applies = 0;
    KsClock clk;

    double& Tm(int r, int c) { return T[(size_t)c * ldt + r]; }
    // injects the start vector, sizes the host arrays
    int init(const S* v0) {
        m = b.m;
        n = b.n;
        max_out = std::min(max_out, m);
        nev = std::min<int>(o->nev, m);
        keep_fraction = ks_keep_fraction(o);
        rng = ks_rng(o);
        vec.resize((size_t)n);
        if (v0) memcpy(vec.data(), v0, (size_t)n * sizeof(S));
        else b.random(rng, vec);
        LSA_CHECK(b.inject(0, vec.data()));
        ldt = m + 1;
        T.assign((size_t)ldt * m, 0.0);
        Y.resize((size_t)m * m);
        for (auto* a : {&theta, &est, &rel, &keys}) a->resize((size_t)m);
        rank.resize((size_t)m);
        memset(result, 0, sizeof *result);
        return LSA_OK;
    }
    int inject_random(int j) {
        b.random(rng, vec);
        return b.inject(j, vec.data());
    }
    // the expansion from `kept` to m vectors
    int expand() {
        clk.start();
        LSA_CHECK(ks_expand(kept, m, &applies, [&](int j, int32_t* bd) { return b.extend(j, T.data(), ldt, bd); }, [&](int j) { return inject_random(j); }));
        clk.lap(clk.expand);
        return LSA_OK;
    }
    // The expansion whose first run of steps a lockstep driver has made (its status and breakdown step, `seconds` of wall time booked
    // to this problem): what follows a breakdown -- the fresh direction, the rest of the steps -- is the solo code's.  *later_steps:
    // the steps the solo code ran here after that first run (none unless it broke down).
    int expand_after(int rc0, int32_t bd0, double seconds, int64_t* later_steps) {
        bool first = true;
        const int64_t before = applies + (bd0 < 0 ? m - kept : bd0 - kept + 1);
        *later_steps = 0;
        clk.start();
        LSA_CHECK(ks_expand(kept, m, &applies,
                            [&](int j, int32_t* bd) {
                                if (!first) return b.extend(j, T.data(), ldt, bd);
                                first = false;
                                LSA_CHECK(rc0);
                                *bd = bd0;
                                return (int)LSA_OK;
                            },
                            [&](int j) { return inject_random(j); }));
        clk.lap(clk.expand);
        clk.expand += seconds;
        *later_steps = applies - before;
        return LSA_OK;
    }
    // The body of the loop after an expansion: Ritz pairs, convergence test, then either the result (*done) or the restart.
    int after_expand(bool* done) {
        *done = false;
        clk.start();
        const double beta = Tm(m, m - 1);
        for (int c = 0; c < m; ++c)
            for (int r = 0; r < m; ++r) Y[(size_t)c * m + r] = Tm(r, c);
        // ---- Ritz pairs and residual estimates ----
        if (!sym_eig(m, Y.data(), m, theta.data()))
            return lsa_set_error(ctx, LSA_ERR_DIVERGED, "Lanczos: the QL algorithm on the projected matrix did not converge");
        for (int c = 0; c < m; ++c) {
            est[(size_t)c] = std::fabs(beta * Y[(size_t)c * m + (m - 1)]);
            keys[(size_t)c] = b.key(theta[(size_t)c]);
            rel[(size_t)c] = est[(size_t)c] / std::max(std::fabs(theta[(size_t)c]), 2.2250738585072014e-308);
        }
        const int nconv = ks_rank_converged(m, keys, rel, o->tol, rank);
        if (nconv >= nev || nconv >= m || restarts >= o->max_restarts) {
            const int nout = std::min<int>(nconv, max_out);
            if (nout > 0) {
                std::vector<double> Yo((size_t)m * nout);
                for (int c = 0; c < nout; ++c) {
                    const int src = rank[(size_t)c];
                    memcpy(&Yo[(size_t)c * m], &Y[(size_t)src * m], (size_t)m * sizeof(double));
                    theta_out[c] = theta[(size_t)src];
                    lambda_out[c] = b.back(theta[(size_t)src]);
                    if (est_out) est_out[c] = rel[(size_t)src];
                }
                clk.lap(clk.dense);
                if (X_out) LSA_CHECK(b.vectors(nout, Yo.data(), lambda_out, X_out));
                clk.lap(clk.restart);
            }
            clk.lap(clk.dense);
            ks_fill_result(result, clk, nconv, nout, restarts, applies, nconv < m ? rel[(size_t)rank[(size_t)nconv]] : 0.0);
            *done = true;
            return LSA_OK;
        }
        // ---- keep the wanted Ritz vectors and restart: T <- diag(theta_kept) with the spike beta y_{m,i} in row and column knew ----
        const int knew = ks_keep_count(m, nconv, keep_fraction);
        std::vector<double> Yk((size_t)m * knew);
        for (int c = 0; c < knew; ++c) memcpy(&Yk[(size_t)c * m], &Y[(size_t)rank[(size_t)c] * m], (size_t)m * sizeof(double));
        clk.lap(clk.dense);
        LSA_CHECK(b.restart(knew, Yk.data()));
        clk.lap(clk.restart);
        std::fill(T.begin(), T.end(), 0.0);
        for (int c = 0; c < knew; ++c) {
            const int src = rank[(size_t)c];
            Tm(c, c) = theta[(size_t)src];
            const double spike = beta * Y[(size_t)src * m + (m - 1)];
            Tm(knew, c) = spike;
            Tm(c, knew) = spike;
        }
        kept = knew;
        ++restarts;
        return LSA_OK;
    }
};

template <class Basis>
int trl_solve(lsa_ctx* ctx, Basis& b, const lsa_ks_options* o, const typename Basis::scalar* v0, int32_t max_out, double* theta_out,
              double* lambda_out, typename Basis::scalar* X_out, double* est_out, lsa_ks_result* result) {
    TrlState<Basis> st{ctx, b, o, max_out, theta_out, lambda_out, X_out, est_out, result};
    LSA_CHECK(st.init(v0));
    for (bool done = false; !done;) {
        LSA_CHECK(st.expand());
        LSA_CHECK(st.after_expand(&done));
    }
    return LSA_OK;
}

}  // namespace

// Z = Mh^-1 Ah (r x r complex, column-major, leading dimension r) by LU with partial pivoting; Mh and Ah are overwritten (Ah by Z).
// false: Mh is singular.  The reduced problem of the region eigensolver (contour.hip).
bool dense_lu_solve(int32_t r, void* Mh_, void* Ah_) {
    typedef std::complex<double> ci_z;
    ci_z *Mh = (ci_z*)Mh_, *Ah = (ci_z*)Ah_;
    for (int32_t c = 0; c < r; ++c) {
        int32_t piv = c;
        for (int32_t i = c + 1; i < r; ++i)
            if (std::abs(Mh[(size_t)c * r + i]) > std::abs(Mh[(size_t)c * r + piv])) piv = i;
        if (!(std::abs(Mh[(size_t)c * r + piv]) > 0.0)) return false;
        if (piv != c)
            for (int32_t j = 0; j < r; ++j) {
                std::swap(Mh[(size_t)j * r + c], Mh[(size_t)j * r + piv]);
                std::swap(Ah[(size_t)j * r + c], Ah[(size_t)j * r + piv]);
            }
        const ci_z d = Mh[(size_t)c * r + c];
        for (int32_t i = c + 1; i < r; ++i) {
            const ci_z l = Mh[(size_t)c * r + i] / d;
            if (l == ci_z(0.0, 0.0)) continue;
            for (int32_t j = c + 1; j < r; ++j) Mh[(size_t)j * r + i] -= l * Mh[(size_t)j * r + c];
            for (int32_t j = 0; j < r; ++j) Ah[(size_t)j * r + i] -= l * Ah[(size_t)j * r + c];
        }
    }
    for (int32_t j = 0; j < r; ++j)
        for (int32_t i = r - 1; i >= 0; --i) {
            ci_z v = Ah[(size_t)j * r + i];
            for (int32_t k = i + 1; k < r; ++k) v -= Mh[(size_t)k * r + i] * Ah[(size_t)j * r + k];
            Ah[(size_t)j * r + i] = v / Mh[(size_t)i * r + i];
        }
    return true;
}

extern "C" {

int lsa_dense_schur(int32_t n, void* A, int32_t lda, void* Q, int32_t ldq) {
    if (n < 0 || !A || !Q || lda < std::max(1, n) || ldq < std::max(1, n)) return LSA_ERR_ARG;
    return schur(n, Mat{(Z*)A, lda}, Mat{(Z*)Q, ldq}) ? LSA_OK : LSA_ERR_DIVERGED;
}

int lsa_dense_schur_reorder(int32_t n, void* T, int32_t ldt, void* Q, int32_t ldq, const int32_t* select, int32_t* nselected) {
    if (n < 0 || !T || !Q || !select || ldt < std::max(1, n) || ldq < std::max(1, n)) return LSA_ERR_ARG;
    std::vector<char> sel((size_t)n);
    for (int32_t k = 0; k < n; ++k) sel[(size_t)k] = select[k] != 0;
    const int ks = schur_reorder(n, Mat{(Z*)T, ldt}, Mat{(Z*)Q, ldq}, sel);
    if (nselected) *nselected = ks;
    return LSA_OK;
}

int lsa_dense_tri_eigenvectors(int32_t n, const void* T, int32_t ldt, void* S, int32_t lds) {
    if (n < 0 || !T || !S || ldt < std::max(1, n) || lds < std::max(1, n)) return LSA_ERR_ARG;
    tri_eigenvectors(n, Mat{(Z*)T, ldt}, Mat{(Z*)S, lds});
    return LSA_OK;
}

// ---- inertia of a dense real symmetric matrix (host): Bunch-Kaufman diagonal pivoting -------------------------------------
// What SLEPc's spectrum slicing asks of the factorisation behind set_interval / iEpsWhich.ALL (Solver/utils.py:248-254): the
// number of negative eigenvalues of A - sigma M = the number of eigenvalues of the definite pencil below sigma (Sylvester).  The
// multifrontal LU is a block congruence C = L D L^T with D = diag(pivot blocks) when C is symmetric, so the inertia of C is the
// sum over the tree nodes of the inertia of their (dense, symmetric) pivot blocks -- lsa_ndlu_inertia hands them to this routine.
// A = P L D L^T P^T with 1 x 1 and 2 x 2 diagonal blocks in D (a 2 x 2 block of the algorithm has one eigenvalue of each sign);
// the whole symmetric matrix is kept and updated (the pivot blocks of a forest are a few hundred rows; O(2 n^3 / 3)).
// Pivots below tol_rel * max|A| count as zero.  Returns negative / zero / positive counts.
int lsa_dense_sym_inertia(int32_t n, const double* A, int32_t lda, double tol_rel, int64_t* negative, int64_t* zero, int64_t* positive) {
    if (n < 0 || (n > 0 && !A) || lda < std::max(1, n) || !negative || !zero || !positive) return LSA_ERR_ARG;
    *negative = *zero = *positive = 0;
    if (n == 0) return LSA_OK;
    std::vector<double> w((size_t)n * n);
    double amax = 0.0;
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i) {
            const double v = 0.5 * (A[(size_t)j * lda + i] + A[(size_t)i * lda + j]);  // (rounding leaves a computed inverse unsymmetric in the last bits)
            if (!std::isfinite(v)) return LSA_ERR_NONFINITE;
            w[(size_t)j * n + i] = v;
            amax = std::max(amax, std::fabs(v));
        }
    auto W = [&](int i, int j) -> double& { return w[(size_t)j * n + i]; };
    auto swap_sym = [&](int p, int q) {  // rows and columns p <-> q of the symmetric matrix
        if (p == q) return;
        for (int j = 0; j < n; ++j) std::swap(W(p, j), W(q, j));
        for (int i = 0; i < n; ++i) std::swap(W(i, p), W(i, q));
    };
    const double alpha = (1.0 + std::sqrt(17.0)) / 8.0, tiny = std::max(tol_rel, 0.0) * amax;
    int k = 0;
    while (k < n) {
        const double absakk = std::fabs(W(k, k));
        int imax = k;
        double colmax = 0.0;
        for (int i = k + 1; i < n; ++i)
            if (std::fabs(W(i, k)) > colmax) colmax = std::fabs(W(i, k)), imax = i;
        int step = 1;
        if (std::max(absakk, colmax) <= tiny) {  // the whole column vanishes: a zero eigenvalue (to the tolerance)
            ++*zero;
            ++k;
            continue;
        }
        if (absakk < alpha * colmax) {
            double rowmax = 0.0;
            for (int j = k; j < n; ++j)
                if (j != imax) rowmax = std::max(rowmax, std::fabs(W(imax, j)));
            if (absakk >= alpha * colmax * (colmax / rowmax)) {
                // 1 x 1 pivot in place
            } else if (std::fabs(W(imax, imax)) >= alpha * rowmax) {
                swap_sym(k, imax);  // 1 x 1 pivot, the diagonal entry of row imax
            } else {
                swap_sym(k + 1, imax);  // 2 x 2 pivot: rows k and imax
                step = 2;
            }
        }
        if (step == 1) {
            const double d = W(k, k);
            if (std::fabs(d) <= tiny) ++*zero;
            else if (d < 0.0) ++*negative;
            else ++*positive;
            if (std::fabs(d) > tiny) {
                const double dinv = 1.0 / d;
                for (int j = k + 1; j < n; ++j) {
                    const double f = W(k, j) * dinv;
                    if (f == 0.0) continue;
                    for (int i = k + 1; i < n; ++i) W(i, j) -= W(i, k) * f;
                }
            }
        } else {
            // D = [a b; b c] with |b| the largest entry of its rows: det < 0, one eigenvalue of each sign
            const double a = W(k, k), b = W(k + 1, k), c = W(k + 1, k + 1), det = a * c - b * b;
            if (std::fabs(det) <= tiny * tiny) {
                *zero += 2;
            } else {
                if (det < 0.0) {
                    ++*negative;
                    ++*positive;
                } else if (a + c < 0.0) *negative += 2;
                else *positive += 2;
                for (int j = k + 2; j < n; ++j) {
                    // column j of the update: W22 -= W21 D^-1 W12
                    const double u = W(k, j), v = W(k + 1, j);
                    const double f0 = (c * u - b * v) / det, f1 = (a * v - b * u) / det;
                    if (f0 == 0.0 && f1 == 0.0) continue;
                    for (int i = k + 2; i < n; ++i) W(i, j) -= W(i, k) * f0 + W(i, k + 1) * f1;
                }
            }
        }
        k += step;
    }
    return LSA_OK;
}

static_assert(sizeof(lsa_ks_result) == 56 && sizeof(lsa_ks_options) == 88, "lsa_ks_options layout is part of the C-ABI (tests/test_abi.py)");

}  // extern "C"

namespace {

// What the Krylov-Schur iteration keeps per problem: the projected matrix and its Schur form, the vectors kept, the counters, the
// clock, the generator and the result.  lsa_krylov_solve is the loop over one state, lsa_krylov_solve_batch the loop over J.
struct KsState {
    lsa_ctx* ctx;
    lsa_krylov* k;
    const lsa_ks_options* o;
    const double* mask;
    int32_t max_out;
    void *theta_out, *lambda_out, *X_out;
    double* est_out;
    lsa_ks_result* result;
    int32_t m = 0;
    int64_t n = 0;
    int nev = 0, ldh = 0;
    double keep_fraction = 0.5;
    Selector sel;
    Rng rng;
    std::vector<Z> vec, H, T, Q, S, b, bq, w;
    std::vector<double> est, rel, keys;
    std::vector<int> rank;
    std::vector<char> select;
    int kept = 0, restarts = 0;
    int64_t applies = 0;
    KsClock clk;
    bool ahead = false;  // solo loop: the next cycle's first operator apply is queued before the dense phase (krylov_preapply)

    void random_vector() {
        for (int64_t i = 0; i < n; ++i) {
            rng.normal_pair(vec[(size_t)i].re, vec[(size_t)i].im);
            if (mask && mask[i] == 0.0) vec[(size_t)i] = {0.0, 0.0};
        }
    }
    // checks the arguments, injects the start vector, sizes the host arrays
    int init(const char* who, const void* v0) {
        LSA_CHECK(lsa_krylov_shape(k, &n, &m));
        if (m > n) return lsa_set_error(ctx, LSA_ERR_ARG, "ncv = %d exceeds the problem size %lld", m, (long long)n);
        LSA_CHECK(ks_check_options(ctx, who, o, max_out, theta_out, lambda_out));
        nev = std::min<int>(o->nev, m);
        keep_fraction = ks_keep_fraction(o);
        sel = Selector{o->which, o->transform, {o->sigma[0], o->sigma[1]}, {o->antishift[0], o->antishift[1]}, {o->target[0], o->target[1]}};
        rng = ks_rng(o);
        vec.resize((size_t)n);
        if (v0) {
            memcpy(vec.data(), v0, (size_t)n * sizeof(Z));
            if (mask)
                for (int64_t i = 0; i < n; ++i)
                    if (mask[i] == 0.0) vec[(size_t)i] = {0.0, 0.0};
        } else {
            random_vector();
        }
        LSA_CHECK(lsa_krylov_inject(ctx, k, 0, vec.data()));
        ldh = m + 1;
        H.assign((size_t)ldh * m, Z{0.0, 0.0});
        for (auto* a : {&T, &Q, &S}) a->resize((size_t)m * m);
        for (auto* a : {&b, &bq, &w}) a->resize((size_t)m);
        for (auto* a : {&est, &rel, &keys}) a->resize((size_t)m);
        rank.resize((size_t)m);
        select.resize((size_t)m);
        memset(result, 0, sizeof *result);
        return LSA_OK;
    }
    int extend(int j, int32_t* bd) {
        LSA_CHECK(lsa_krylov_extend(ctx, k, j, m, H.data(), ldh, bd));
        if (*bd >= 0) H[(size_t)*bd * ldh + (size_t)*bd + 1] = {0.0, 0.0};
        return (int)LSA_OK;
    }
    int inject_random(int j) {
        random_vector();
        return lsa_krylov_inject(ctx, k, j, vec.data());
    }
    // the expansion from `kept` to m vectors through the solo code
    int expand() {
        clk.start();
        krylov_arm_preapply(k, ahead && restarts < o->max_restarts);  // (the last cycle allowed ends in the result: nothing follows it)
        LSA_CHECK(ks_expand(kept, m, &applies, [&](int j, int32_t* bd) { return extend(j, bd); }, [&](int j) { return inject_random(j); }));
        clk.lap(clk.expand);
        return LSA_OK;
    }
    // The expansion whose first run of steps the lockstep driver has made (its status and breakdown step, `seconds` of wall time
    // booked to this problem): what follows a breakdown -- the fresh direction, the rest of the steps -- is the solo code's.
    // *later_steps: the steps the solo code ran here after that first run (none unless it broke down).
    int expand_after(int rc0, int32_t bd0, double seconds, int64_t* later_steps) {
        bool first = true;
        const int64_t before = applies + (bd0 < 0 ? m - kept : bd0 - kept + 1);
        *later_steps = 0;
        clk.start();
        LSA_CHECK(ks_expand(kept, m, &applies,
                            [&](int j, int32_t* bd) {
                                if (!first) return extend(j, bd);
                                first = false;
                                LSA_CHECK(rc0);
                                *bd = bd0;
                                if (*bd >= 0) H[(size_t)*bd * ldh + (size_t)*bd + 1] = {0.0, 0.0};
                                return (int)LSA_OK;
                            },
                            [&](int j) { return inject_random(j); }));
        clk.lap(clk.expand);
        clk.expand += seconds;
        *later_steps = applies - before;
        return LSA_OK;
    }
    // The body of the loop after an expansion: Ritz pairs, convergence test, then either the result (*done) or the restart.
    int after_expand(const char* who, bool* done) {
        const Mat Hm{H.data(), ldh}, Tm{T.data(), m}, Qm{Q.data(), m}, Sm{S.data(), m};
        *done = false;
        clk.start();
        for (int c = 0; c < m; ++c) {
            b[(size_t)c] = Hm(m, c);  // b^H: the row under the square part
            for (int r = 0; r < m; ++r) Tm(r, c) = Hm(r, c);
        }
        // the final vector's operator apply runs on the device under the Schur form (if this cycle ends the solve, for nothing)
        if (ahead && restarts < o->max_restarts) LSA_CHECK(krylov_preapply(ctx, k, m));
        // ---- Ritz pairs and residual estimates ----
        if (!schur(m, Tm, Qm)) return lsa_set_error(ctx, LSA_ERR_DIVERGED, "Krylov-Schur: the QR algorithm on the projected matrix did not converge");
        tri_eigenvectors(m, Tm, Sm);
        for (int c = 0; c < m; ++c) {
            Z acc = {0.0, 0.0};
            for (int r = 0; r < m; ++r) acc = acc + b[(size_t)r] * Qm(r, c);
            bq[(size_t)c] = acc;
        }
        for (int c = 0; c < m; ++c) {
            Z acc = {0.0, 0.0};
            for (int r = 0; r <= c; ++r) acc = acc + bq[(size_t)r] * Sm(r, c);
            est[(size_t)c] = zabs(acc);
            w[(size_t)c] = Tm(c, c);
            keys[(size_t)c] = sel.key(w[(size_t)c]);
            rel[(size_t)c] = est[(size_t)c] / std::max(zabs(w[(size_t)c]), 2.2250738585072014e-308);
        }
        const int nconv = ks_rank_converged(m, keys, rel, o->tol, rank);
        if (nconv >= nev || nconv >= m || restarts >= o->max_restarts) {
            const int nout = std::min<int>(nconv, max_out);
            if (nout > 0) {
                std::vector<Z> Y((size_t)m * nout);
                for (int c = 0; c < nout; ++c) {
                    const int src = rank[(size_t)c];
                    for (int r = 0; r < m; ++r) {
                        Z acc = {0.0, 0.0};
                        for (int q = 0; q <= src; ++q) acc = acc + Qm(r, q) * Sm(q, src);
                        Y[(size_t)c * m + r] = acc;
                    }
                    ((Z*)theta_out)[c] = w[(size_t)src];
                    ((Z*)lambda_out)[c] = sel.back(w[(size_t)src]);
                    if (est_out) est_out[c] = rel[(size_t)src];
                }
                clk.lap(clk.dense);
                if (X_out) LSA_CHECK(lsa_krylov_ritz_vectors(ctx, k, m, nout, Y.data(), m, 3, X_out));
                clk.lap(clk.restart);
            }
            clk.lap(clk.dense);
            ks_fill_result(result, clk, nconv, nout, restarts, applies, nconv < m ? rel[(size_t)rank[(size_t)nconv]] : 0.0);
            *done = true;
            return k_agree_in_step(ctx, who);  // (a sharded solve ends with the ranks comparing their exchange counts)
        }
        // ---- truncate to the wanted part of the Schur form and restart ----
        int knew = ks_keep_count(m, nconv, keep_fraction);
        {
            // ties at the selection threshold are all selected (what a sort callback of the Schur routine would do)
            std::vector<double> sorted(keys);
            std::sort(sorted.begin(), sorted.end());
            const double thr = sorted[(size_t)knew] > sorted[(size_t)knew - 1] ? 0.5 * (sorted[(size_t)knew - 1] + sorted[(size_t)knew]) : sorted[(size_t)knew - 1];
            for (int c = 0; c < m; ++c) select[(size_t)c] = keys[(size_t)c] <= thr;
            const int sdim = schur_reorder(m, Tm, Qm, select);
            knew = std::max(std::min(sdim, m - 1), 1);
        }
        clk.lap(clk.dense);
        LSA_CHECK(ahead ? krylov_restart_queued(ctx, k, m, knew, Q.data(), m) : lsa_krylov_restart(ctx, k, m, knew, Q.data(), m));
        clk.lap(clk.restart);
        std::fill(H.begin(), H.end(), Z{0.0, 0.0});
        for (int c = 0; c < knew; ++c) {
            for (int r = 0; r <= c; ++r) Hm(r, c) = Tm(r, c);
            Z acc = {0.0, 0.0};
            for (int r = 0; r < m; ++r) acc = acc + b[(size_t)r] * Qm(r, c);
            Hm(knew, c) = acc;
        }
        kept = knew;
        ++restarts;
        return LSA_OK;
    }
};

}  // namespace

extern "C" {

int lsa_krylov_solve(lsa_ctx* ctx, lsa_krylov* k, const lsa_ks_options* o, const void* v0, const double* mask, int32_t max_out, void* theta_out,
                     void* lambda_out, void* X_out, double* est_out, lsa_ks_result* result) {
    if (!ctx || !k || !o || !result) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_krylov_solve: null argument");
    KsState st{ctx, k, o, mask, max_out, theta_out, lambda_out, X_out, est_out, result};
    LSA_CHECK(st.init("lsa_krylov_solve", v0));
    st.ahead = true;
    int rc = LSA_OK;
    for (bool done = false; !done && rc == LSA_OK;) {
        rc = st.expand();
        if (rc == LSA_OK) rc = st.after_expand("lsa_krylov_solve", &done);
    }
    krylov_arm_preapply(k, false);
    return rc;
}

static_assert(sizeof(lsa_ks_batch_info) == 288, "lsa_ks_batch_info layout is part of the C-ABI (tests/test_lockstep_cpu.py)");
static_assert(sizeof(((lsa_ks_batch_info*)nullptr)->lockstep_steps) == 8 * kKrylovGroupMax && sizeof(((lsa_ks_batch_info*)nullptr)->solo_steps) == 8 * kKrylovGroupMax,
              "the per-problem counters of lsa_ks_batch_info hold one entry per problem of a group");

int lsa_krylov_solve_batch(lsa_ctx* ctx, int32_t J, lsa_krylov* const* k, const lsa_ks_options* const* opts, const void* const* v0, int32_t max_out,
                           void* const* theta_out, void* const* lambda_out, void* const* X_out, double* const* est_out, lsa_ks_result* results,
                           int32_t* status, lsa_ks_batch_info* info) {
    if (!ctx || !k || !opts || !results || !status) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_krylov_solve_batch: null argument");
    if (J < 1 || J > kKrylovGroupMax) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_krylov_solve_batch: J = %d outside [1, %d]", J, kKrylovGroupMax);
    if (max_out > 0 && (!theta_out || !lambda_out)) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_krylov_solve_batch: output buffers are required");
    for (int32_t z = 0; z < J; ++z)
        if (!opts[z]) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_krylov_solve_batch: null options (problem %d)", z);
    LSA_CHECK(krylov_group_check(ctx, J, k));
    if (info) memset(info, 0, sizeof *info);
    std::vector<KsState> st;
    st.reserve((size_t)J);
    uint8_t active[kKrylovGroupMax] = {};
    int32_t kept[kKrylovGroupMax] = {}, bd[kKrylovGroupMax], erc[kKrylovGroupMax];
    void* Hs[kKrylovGroupMax] = {};
    int32_t nactive = 0;
    std::string errs[kKrylovGroupMax];     // the error text of every problem that failed
    auto leave = [&](int32_t z, int rc) {  // problem z is done: with its result, or with its own error
        if (rc != LSA_OK && status[z] == LSA_OK) {
            status[z] = rc;
            if (errs[z].empty()) errs[z] = ctx->err;  // (krylov_extend_batch has left the text of its own errors)
        }
        nactive -= active[z];
        active[z] = 0;
    };
    for (int32_t z = 0; z < J; ++z) {
        status[z] = LSA_OK;
        st.push_back(KsState{ctx, k[z], opts[z], nullptr, max_out, theta_out ? theta_out[z] : nullptr, lambda_out ? lambda_out[z] : nullptr,
                             X_out ? X_out[z] : nullptr, est_out ? est_out[z] : nullptr, &results[z]});
        active[z] = 1;
        ++nactive;
        const int rc = st[(size_t)z].init("lsa_krylov_solve_batch", v0 ? v0[z] : nullptr);
        if (rc != LSA_OK) {
            lsa_name_problem(ctx, z);
            leave(z, rc);
        }
        Hs[z] = st[(size_t)z].H.data();
    }
    KrylovGroupBuf gb;
    int grc = nactive > 0 ? krylov_group_alloc(ctx, J, k, &gb) : (memset(&gb, 0, sizeof gb), (int)LSA_OK);
    while (grc == LSA_OK && nactive > 0) {
        const int32_t m = st[0].m, na = nactive;
        for (int32_t z = 0; z < J; ++z) kept[z] = st[(size_t)z].kept;
        const double t0 = now_s();
        grc = krylov_extend_batch(ctx, &gb, k, active, kept, m, Hs, m + 1, bd, erc, errs, info);
        if (grc != LSA_OK) break;
        const double share = (now_s() - t0) / na;
        for (int32_t z = 0; z < J; ++z) {
            if (!active[z]) continue;
            KsState& s = st[(size_t)z];
            bool done = false;
            int64_t later = 0;
            int rc = s.expand_after(erc[z], bd[z], share, &later);
            if (info) info->solo_steps[z] += later;  // (what followed a breakdown: the solo code's steps too)
            if (rc == LSA_OK) rc = s.after_expand("lsa_krylov_solve_batch", &done);
            if (rc != LSA_OK && erc[z] == LSA_OK) lsa_name_problem(ctx, z);  // (krylov_extend_batch has named its own)
            if (rc != LSA_OK || done) leave(z, rc);
        }
    }
    krylov_group_free(&gb);
    if (info && info->rounds > 0) info->launches_per_round = (double)info->launches / (double)info->rounds;
    if (grc != LSA_OK) {  // the group's own buffers could not be had: an error of every problem that was still going
        for (int32_t z = 0; z < J; ++z)
            if (active[z]) status[z] = grc;
        return grc;
    }
    // the context's error text: those of all failed problems in problem order, each naming its problem (the first one's leads)
    int first_rc = LSA_OK;
    std::string all;
    for (int32_t z = 0; z < J; ++z)
        if (status[z] != LSA_OK) {
            if (first_rc == LSA_OK) first_rc = status[z];
            else all += "; ";
            all += errs[z];
        }
    if (first_rc != LSA_OK) ctx->err = all;
    return first_rc;
}

int lsa_eigs_sinvert(lsa_ctx* ctx, const lsa_mat* A, const lsa_mat* M, const double sigma[2], int32_t nev, int32_t ncv, double tol, int32_t max_restarts,
                     const lsa_op_options* opts, const void* v0, const int32_t* row_perm, int32_t max_out, void* lambda_out, void* X_out, double* est_out,
                     lsa_ks_result* result, lsa_stats* stats) {
    if (!ctx || !A || !sigma || !opts || !result) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_eigs_sinvert: null argument");
    if (ncv <= 0) ncv = std::max(2 * nev, nev + 15);
    ncv = (int32_t)std::min<int64_t>(ncv, lsa_mat_rows(A));
    lsa_op* op = nullptr;
    lsa_krylov* kr = nullptr;
    int rc = lsa_op_create(ctx, A, M, sigma, 0, opts, &op);
    if (rc == LSA_OK) rc = lsa_krylov_create(ctx, op, ncv, &kr);
    if (rc == LSA_OK && row_perm) rc = lsa_krylov_set_row_permutation(ctx, kr, row_perm);
    if (rc == LSA_OK) {
        lsa_ks_options o;
        memset(&o, 0, sizeof o);
        o.nev = nev;
        o.max_restarts = max_restarts;
        o.tol = tol;
        o.which = LSA_WHICH_TARGET_MAGNITUDE;
        o.transform = 0;
        o.sigma[0] = o.target[0] = sigma[0];
        o.sigma[1] = o.target[1] = sigma[1];
        o.keep_fraction = 0.5;
        std::vector<Z> theta((size_t)std::max(max_out, 1));
        rc = lsa_krylov_solve(ctx, kr, &o, v0, nullptr, max_out, theta.data(), lambda_out, X_out, est_out, result);
    }
    if (op && stats) (void)lsa_op_stats(op, stats);
    if (kr) lsa_krylov_destroy(kr);
    if (op) lsa_op_destroy(op);
    return rc;
}

int lsa_dense_syev(int32_t n, double* A, int32_t lda, double* w) {
    if (n < 0 || (n > 0 && (!A || !w)) || lda < std::max(1, n)) return LSA_ERR_ARG;
    for (int j = 0; j < n; ++j)
        for (int i = j; i < n; ++i)
            if (!std::isfinite(A[(size_t)j * lda + i])) return LSA_ERR_NONFINITE;
    return sym_eig(n, A, lda, w) ? LSA_OK : LSA_ERR_DIVERGED;
}

// Thick-restart Lanczos = the symmetric variant of Krylov-Schur (SLEPc's EPSSolve_KrylovSchur_Symm behind EPS_GHEP / EPS_HEP): the
// loop of lsa_krylov_solve with a real M-orthonormal basis (lanczos.hip), a real symmetric projected matrix T (after a restart:
// diag(theta_1..theta_k) with the spike beta y_{m,i} in row and column k, tridiagonal behind it) and lsa_dense_syev in place of the
// complex Schur form.  The loop itself is trl_solve (above), which the resolvent iteration shares.
int lsa_lanczos_solve(lsa_ctx* ctx, lsa_lanczos* l, const lsa_ks_options* o, const double* v0, int32_t max_out, double* theta_out,
                      double* lambda_out, double* X_out, double* est_out, lsa_ks_result* result) {
    if (!ctx || !l || !o || !result) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_lanczos_solve: null argument");
    TrlRealBasis b{ctx, l, Selector{}};
    LSA_CHECK(lanczos_shape(l, &b.n, &b.m));
    LSA_CHECK(ks_check_options(ctx, "lsa_lanczos_solve", o, max_out, theta_out, lambda_out));
    if (o->transform != 0 || o->sigma[1] != 0.0 || o->target[1] != 0.0)
        return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_lanczos_solve: shift-invert (transform 0) with a real shift and a real target only");
    switch (o->which) {
        case LSA_WHICH_TARGET_MAGNITUDE: case LSA_WHICH_TARGET_REAL: case LSA_WHICH_LARGEST_MAGNITUDE: case LSA_WHICH_LARGEST_REAL:
        case LSA_WHICH_SMALLEST_REAL: break;
        default: return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_lanczos_solve: which = %d has no meaning for a real spectrum", o->which);
    }
    b.sel = Selector{o->which, 0, {o->sigma[0], 0.0}, {0.0, 0.0}, {o->target[0], 0.0}};
    return trl_solve(ctx, b, o, v0, max_out, theta_out, lambda_out, X_out, est_out, result);
}

// The resolvent iteration (resolvent.hip): the same loop on the basis with complex scalars, for W = C^-1 M C^-H M; theta_j = sigma_j^2, largest first.
int lsa_resolvent_solve(lsa_ctx* ctx, lsa_resolvent* r, const lsa_ks_options* o, const void* v0, int32_t max_out, double* theta_out,
                        double* gain_out, void* Q_out, void* F_out, double* est_out, lsa_ks_result* result, int64_t* counts) {
    if (!ctx || !r || !o || !result) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_resolvent_solve: null argument");
    if (F_out && !Q_out) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_resolvent_solve: the forcings are computed from the responses: F_out needs Q_out");
    TrlResolventBasis b{ctx, r, (cplx*)F_out};
    LSA_CHECK(resolvent_shape(r, &b.n, &b.m));
    LSA_CHECK(ks_check_options(ctx, "lsa_resolvent_solve", o, max_out, theta_out, gain_out));
    const int rc = trl_solve(ctx, b, o, (const cplx*)v0, max_out, theta_out, gain_out, (cplx*)Q_out, est_out, result);
    if (counts) resolvent_counts(r, counts);
    return rc;
}

// The same iteration for J frequencies of one sweep at once: the loop over J states, their expansions through resolvent_extend_batch
// (one batched launch per launch of a solo step and one read-back per round for the members in lockstep, the solo code for the others),
// everything after an expansion per member through the state's own method.  A member that is done forms its vectors and forcings on
// its own factor set and leaves while the rest go on.
int lsa_resolvent_solve_batch(lsa_ctx* ctx, int32_t J, lsa_resolvent* const* rs, const lsa_ks_options* const* opts, const void* const* v0, int32_t max_out,
                              double* const* theta_out, double* const* gain_out, void* const* Q_out, void* const* F_out, double* const* est_out,
                              lsa_ks_result* results, int64_t* counts, int32_t* status, lsa_ks_batch_info* info) {
    const char* who = "lsa_resolvent_solve_batch";
    if (!ctx || !rs || !opts || !results || !status) return lsa_set_error(ctx, LSA_ERR_ARG, "%s: null argument", who);
    LSA_CHECK(resolvent_group_check(ctx, who, J, rs));
    if (max_out > 0 && (!theta_out || !gain_out)) return lsa_set_error(ctx, LSA_ERR_ARG, "%s: output buffers are required", who);
    for (int32_t z = 0; z < J; ++z) {
        if (!opts[z]) return lsa_set_error(ctx, LSA_ERR_ARG, "%s: null options (problem %d)", who, z);
        if (F_out && F_out[z] && !(Q_out && Q_out[z]))
            return lsa_set_error(ctx, LSA_ERR_ARG, "%s: the forcings are computed from the responses: F_out needs Q_out (problem %d)", who, z);
    }
    if (info) memset(info, 0, sizeof *info);
    typedef TrlState<TrlResolventBasis> State;
    std::vector<State> st;
    st.reserve((size_t)J);
    uint8_t active[kKrylovGroupMax] = {};
    int32_t kept[kKrylovGroupMax] = {}, bd[kKrylovGroupMax], erc[kKrylovGroupMax];
    double* Ts[kKrylovGroupMax] = {};
    int32_t nactive = 0;
    std::string errs[kKrylovGroupMax];     // the error text of every problem that failed
    auto leave = [&](int32_t z, int rc) {  // problem z is done: with its result, or with its own error
        if (rc != LSA_OK && status[z] == LSA_OK) {
            status[z] = rc;
            if (errs[z].empty()) errs[z] = ctx->err;  // (resolvent_extend_batch has left the text of its own errors)
        }
        nactive -= active[z];
        active[z] = 0;
    };
    for (int32_t z = 0; z < J; ++z) {
        status[z] = LSA_OK;
        TrlResolventBasis b{ctx, rs[z], F_out ? (cplx*)F_out[z] : nullptr};
        (void)resolvent_shape(rs[z], &b.n, &b.m);
        st.push_back(State{ctx, b, opts[z], max_out, theta_out ? theta_out[z] : nullptr, gain_out ? gain_out[z] : nullptr, Q_out ? (cplx*)Q_out[z] : nullptr,
                           est_out ? est_out[z] : nullptr, &results[z]});
        memset(&results[z], 0, sizeof results[z]);
        active[z] = 1;
        ++nactive;
        int rc = ks_check_options(ctx, who, opts[z], max_out, st[(size_t)z].theta_out, st[(size_t)z].lambda_out);
        if (rc == LSA_OK) rc = st[(size_t)z].init(v0 ? (const cplx*)v0[z] : nullptr);
        if (rc != LSA_OK) {
            lsa_name_problem(ctx, z);
            leave(z, rc);
        }
        Ts[z] = st[(size_t)z].T.data();
    }
    LanczosGroupBuf gb;
    int grc = nactive > 0 ? resolvent_group_alloc(ctx, J, rs, &gb) : (memset(&gb, 0, sizeof gb), (int)LSA_OK);
    while (grc == LSA_OK && nactive > 0) {
        const int32_t m = st[0].b.m;
        for (int32_t z = 0; z < J; ++z) kept[z] = st[(size_t)z].kept;
        const int32_t na = nactive;
        const double t0 = now_s();
        grc = resolvent_extend_batch(ctx, &gb, J, rs, active, kept, m, Ts, m + 1, bd, erc, errs, info);
        if (grc != LSA_OK) break;
        const double share = (now_s() - t0) / na;
        for (int32_t z = 0; z < J; ++z) {
            if (!active[z]) continue;
            State& s = st[(size_t)z];
            bool done = false;
            int64_t later = 0;
            int rc = s.expand_after(erc[z], bd[z], share, &later);
            if (info) info->solo_steps[z] += later;  // (what followed a breakdown: the solo code's steps too)
            if (rc == LSA_OK) rc = s.after_expand(&done);
            if (rc != LSA_OK && erc[z] == LSA_OK) lsa_name_problem(ctx, z);  // (resolvent_extend_batch has named its own)
            if (rc != LSA_OK || done) leave(z, rc);
        }
    }
    lanczos_group_free(&gb);
    if (counts)
        for (int32_t z = 0; z < J; ++z) resolvent_counts(rs[z], counts + 4 * (size_t)z);
    if (info && info->rounds > 0) info->launches_per_round = (double)info->launches / (double)info->rounds;
    if (grc != LSA_OK) {  // the group's own buffers could not be had: an error of every problem that was still going
        for (int32_t z = 0; z < J; ++z)
            if (active[z]) status[z] = grc;
        return grc;
    }
    return resolvent_group_status(ctx, J, status, errs);
}

// Transient growth (growth.hip): the same loop on the real basis of W = Phi+ Phi, a march of 2N solves behind every step; theta_j = G_j,
// largest first.
int lsa_growth_solve(lsa_ctx* ctx, lsa_growth* g, const lsa_ks_options* o, const double* v0, int32_t max_out, double* theta_out, double* gain_out,
                     double* Q0_out, double* QT_out, double* energy_out, double* est_out, lsa_ks_result* result, int64_t* counts) {
    if (!ctx || !g || !o || !result) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_growth_solve: null argument");
    if ((QT_out || energy_out) && !Q0_out)
        return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_growth_solve: the responses and energies are marched from the initial conditions: they need Q0_out");
    TrlGrowthBasis b{ctx, g, QT_out, energy_out};
    LSA_CHECK(growth_shape(g, &b.n, &b.m, nullptr));
    LSA_CHECK(ks_check_options(ctx, "lsa_growth_solve", o, max_out, theta_out, gain_out));
    const int rc = trl_solve(ctx, b, o, v0, max_out, theta_out, gain_out, Q0_out, est_out, result);
    if (counts) growth_counts(g, counts);
    return rc;
}

// Stochastic forcing (stochastic.hip): the same loop on the real basis of S = (1 / pi) sum_k w_k Re W(z_k), 2N solves on N kept factor
// sets behind every step; theta_j = the variances, largest first.
int lsa_stochastic_solve(lsa_ctx* ctx, lsa_stochastic* h, const lsa_ks_options* o, const double* v0, int32_t max_out, double* theta_out, double* X_out,
                         double* est_out, lsa_ks_result* result, int64_t* counts) {
    if (!ctx || !h || !o || !result) return lsa_set_error(ctx, LSA_ERR_ARG, "lsa_stochastic_solve: null argument");
    TrlStochasticBasis b{ctx, h};
    LSA_CHECK(stochastic_shape(h, &b.n, &b.m));
    std::vector<double> same((size_t)std::max(max_out, 1));  // (the loop's second copy of the values: no transform maps them)
    LSA_CHECK(ks_check_options(ctx, "lsa_stochastic_solve", o, max_out, theta_out, same.data()));
    const int rc = trl_solve(ctx, b, o, v0, max_out, theta_out, same.data(), X_out, est_out, result);
    if (rc == LSA_OK) stochastic_book_dense(h, result->seconds_dense);
    if (counts) stochastic_counts(h, counts);
    return rc;
}

}  // extern "C"
