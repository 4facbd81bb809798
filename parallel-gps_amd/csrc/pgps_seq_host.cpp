// pgps_seq_host.cpp -- the reference's SEQUENTIAL Kalman filter / RTS smoother
// (pssgp/kalman/sequential.py:11-73; StateSpaceGP(parallel=False), pssgp/model.py:76-79) as
// host C++.  The reference runs this mode on the CPU too (`--device=/cpu:0`,
// experiments/toy_models/speed_and_stability.sh:8).  It is an explicit mode of the API, not a
// fallback: nothing on the parallel=True path ever reaches this file.
#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/pgps.h"
#include "pgps_philox.h"

namespace {

template <typename T>
struct Seq {
    int d;
    std::vector<T> FP, tmp;
    explicit Seq(int d_) : d(d_), FP((size_t)d_ * d_), tmp((size_t)d_ * d_) {}

    // Pp = sym(F P F^T + Q)
    void predict(const T* F, const T* P, const T* Q, T* Pp) {
        for (int i = 0; i < d; ++i)
            for (int j = 0; j < d; ++j) {
                T acc = 0;
                for (int k = 0; k < d; ++k) acc += F[i * d + k] * P[k * d + j];
                FP[i * d + j] = acc;
            }
        for (int i = 0; i < d; ++i)
            for (int j = 0; j < d; ++j) {
                T acc = Q[i * d + j];
                for (int k = 0; k < d; ++k) acc += FP[i * d + k] * F[j * d + k];
                tmp[i * d + j] = acc;
            }
        for (int i = 0; i < d; ++i)
            for (int j = 0; j < d; ++j) Pp[i * d + j] = T(0.5) * (tmp[i * d + j] + tmp[j * d + i]);
    }
};

// sequential.py:11-47.  Rs (N) non-null: the noise variance of step k is Rs[k] (pgps_seq_kf_het_*), read at observed steps only
template <typename T>
int seq_kf(long N, int d, const T* P0, const T* Fs, const T* Qs, const T* H, T R, const T* ys, T* fms, T* fPs,
           double* ll, T* mps, T* Pps, const T* Rs = nullptr) {
    if (N < 1 || d < 1 || !P0 || !Fs || !Qs || !H || !ys || !fms || !fPs) return PGPS_E_INVALID;
    const size_t dd = (size_t)d * d;
    Seq<T> w(d);
    std::vector<T> m(d, T(0)), P(P0, P0 + dd), mp(d), Pp(dd), u(d);
    double ell = 0.0;
    for (long k = 0; k < N; ++k) {
        const T* F = Fs + k * dd;
        const T* Q = Qs + k * dd;
        for (int i = 0; i < d; ++i) {
            T acc = 0;
            for (int j = 0; j < d; ++j) acc += F[i * d + j] * m[j];
            mp[i] = acc;
        }
        w.predict(F, P.data(), Q, Pp.data());
        const T y = ys[k];
        if (y == y) {
            T S = Rs ? Rs[k] : R, yp = 0;
            for (int i = 0; i < d; ++i) {
                T acc = 0;
                for (int j = 0; j < d; ++j) acc += Pp[i * d + j] * H[j];
                u[i] = acc;
            }
            for (int i = 0; i < d; ++i) { S += H[i] * u[i]; yp += H[i] * mp[i]; }
            const double r = double(y) - double(yp);
            ell += -0.5 * (1.8378770664093453 + std::log(double(S)) + r * r / double(S));
            for (int i = 0; i < d; ++i) m[i] = mp[i] + u[i] / S * (y - yp);
            for (int i = 0; i < d; ++i)
                for (int j = 0; j < d; ++j) P[i * d + j] = Pp[i * d + j] - u[i] * u[j] / S;
        } else {
            m = mp;
            P = Pp;
        }
        for (int i = 0; i < d; ++i)
            for (int j = i + 1; j < d; ++j) {
                const T s = T(0.5) * (P[i * d + j] + P[j * d + i]);
                P[i * d + j] = s;
                P[j * d + i] = s;
            }
        for (int i = 0; i < d; ++i) fms[k * d + i] = m[i];
        for (size_t i = 0; i < dd; ++i) fPs[k * dd + i] = P[i];
        if (mps) for (int i = 0; i < d; ++i) mps[k * d + i] = mp[i];
        if (Pps) for (size_t i = 0; i < dd; ++i) Pps[k * dd + i] = Pp[i];
    }
    if (ll) *ll = ell;
    return std::isfinite(ell) ? PGPS_OK : PGPS_E_NUMERIC;
}

// Cholesky solve  X = A^-1 B  (A SPD d x d, B d x d), in place in B.  Returns false if A is not PD.
template <typename T>
bool chol_solve(int d, std::vector<T>& A, T* B) {
    for (int j = 0; j < d; ++j) {
        T s = A[j * d + j];
        for (int k = 0; k < j; ++k) s -= A[j * d + k] * A[j * d + k];
        if (!(s > 0)) return false;
        const T l = std::sqrt(s);
        A[j * d + j] = l;
        for (int i = j + 1; i < d; ++i) {
            T t = A[i * d + j];
            for (int k = 0; k < j; ++k) t -= A[i * d + k] * A[j * d + k];
            A[i * d + j] = t / l;
        }
    }
    for (int c = 0; c < d; ++c) {
        for (int i = 0; i < d; ++i) {
            T t = B[i * d + c];
            for (int k = 0; k < i; ++k) t -= A[i * d + k] * B[k * d + c];
            B[i * d + c] = t / A[i * d + i];
        }
        for (int i = d - 1; i >= 0; --i) {
            T t = B[i * d + c];
            for (int k = i + 1; k < d; ++k) t -= A[k * d + i] * B[k * d + c];
            B[i * d + c] = t / A[i * d + i];
        }
    }
    return true;
}

// sequential.py:50-68
template <typename T>
int seq_ks(long N, int d, const T* Fs, const T* ms, const T* Ps, const T* mps, const T* Pps, T* sms, T* sPs) {
    if (N < 1 || d < 1 || !Fs || !ms || !Ps || !mps || !Pps || !sms || !sPs) return PGPS_E_INVALID;
    const size_t dd = (size_t)d * d;
    std::vector<T> A(dd), Ct(dd), D(dd), X(dd), sm(ms + (N - 1) * d, ms + N * d),
        sP(Ps + (N - 1) * dd, Ps + N * dd);
    for (int i = 0; i < d; ++i) sms[(N - 1) * d + i] = sm[i];
    for (size_t i = 0; i < dd; ++i) sPs[(N - 1) * dd + i] = sP[i];
    for (long k = N - 2; k >= 0; --k) {
        const T* F = Fs + (k + 1) * dd;
        const T* P = Ps + k * dd;
        const T* Pp = Pps + (k + 1) * dd;
        const T* mp = mps + (k + 1) * d;
        for (size_t i = 0; i < dd; ++i) A[i] = Pp[i];
        for (int i = 0; i < d; ++i)
            for (int j = 0; j < d; ++j) {
                T acc = 0;
                for (int l = 0; l < d; ++l) acc += F[i * d + l] * P[l * d + j];
                Ct[i * d + j] = acc;
            }
        if (!chol_solve(d, A, Ct.data())) return PGPS_E_NUMERIC;      // Ct = Pp^-1 F P
        for (int i = 0; i < d; ++i) {
            T acc = ms[k * d + i];
            for (int l = 0; l < d; ++l) acc += Ct[l * d + i] * (sm[l] - mp[l]);
            X[i] = acc;
        }
        for (size_t i = 0; i < dd; ++i) D[i] = sP[i] - Pp[i];
        for (int i = 0; i < d; ++i) sm[i] = X[i];
        for (int i = 0; i < d; ++i)            // X = Ct^T D
            for (int j = 0; j < d; ++j) {
                T acc = 0;
                for (int l = 0; l < d; ++l) acc += Ct[l * d + i] * D[l * d + j];
                X[i * d + j] = acc;
            }
        for (int i = 0; i < d; ++i)
            for (int j = 0; j < d; ++j) {
                T acc = P[i * d + j];
                for (int l = 0; l < d; ++l) acc += X[i * d + l] * Ct[l * d + j];
                A[i * d + j] = acc;
            }
        for (int i = 0; i < d; ++i)
            for (int j = 0; j < d; ++j) sP[i * d + j] = T(0.5) * (A[i * d + j] + A[j * d + i]);
        for (int i = 0; i < d; ++i) sms[k * d + i] = sm[i];
        for (size_t i = 0; i < dd; ++i) sPs[k * dd + i] = sP[i];
    }
    return PGPS_OK;
}

// Semidefinite Cholesky factor of the symmetric M (d x d, full) with diagonal pivoting -- pgps_philox.h psd_chol_columns at
// run-time d: at each step the largest remaining diagonal entry is the pivot (the lowest index on ties), and the factor
// stops (zero columns) when it is not above tau = (d + 3) eps scale (scale = max_i P_ii of the filtered covariance M came from).
// M is consumed; C full, not triangular.
template <typename T>
void psd_chol_rt(int d, T* M, T scale, T* C) {
    const T tau = T(d + 3) * pgps::CholEps<T>::v * scale;
    for (int i = 0; i < d * d; ++i) C[i] = T(0);
    for (int j = 0; j < d; ++j) {
        int p = 0;
        for (int i = 1; i < d; ++i)
            if (M[i * d + i] > M[p * d + p]) p = i;
        if (!(M[p * d + p] > tau)) break;
        const T r = T(1) / std::sqrt(M[p * d + p]);
        for (int i = 0; i < d; ++i) C[i * d + j] = M[i * d + p] * r;
        for (int i = 0; i < d; ++i)
            for (int k = 0; k < d; ++k) M[i * d + k] -= C[i * d + j] * C[k * d + j];
        M[p * d + p] = T(0);
    }
}

// X = A^-1 B (A d x d, B d x d, both overwritten; X in B): Gaussian elimination with partial pivoting.  False if singular.
template <typename T>
bool lu_solve(int d, T* A, T* B) {
    for (int c = 0; c < d; ++c) {
        int piv = c;
        for (int r = c + 1; r < d; ++r)
            if (std::fabs(A[r * d + c]) > std::fabs(A[piv * d + c])) piv = r;
        if (!(A[piv * d + c] != T(0))) return false;
        if (piv != c)
            for (int j = 0; j < d; ++j) { std::swap(A[c * d + j], A[piv * d + j]); std::swap(B[c * d + j], B[piv * d + j]); }
        for (int r = 0; r < d; ++r) {
            if (r == c) continue;
            const T f = A[r * d + c] / A[c * d + c];
            if (f == T(0)) continue;
            for (int j = 0; j < d; ++j) { A[r * d + j] -= f * A[c * d + j]; B[r * d + j] -= f * B[c * d + j]; }
        }
    }
    for (int r = 0; r < d; ++r) {
        const T inv = A[r * d + r];
        for (int j = 0; j < d; ++j) B[r * d + j] /= inv;
    }
    return true;
}

// Backward sampling: x_{N-1} = fm_{N-1} + C(fP_{N-1}) z_{N-1}, x_k = E_k x_{k+1} + g_k + C(L_k) z_k with
// (E_k, g_k, L_k) the smoothing element of step k (E = P F^T Pp^-1, g = m - E F m, L = sym(P - E F P); parallel.py:159-166).
// The element is built once per step for all S samples.  z (S, N, d) or nullptr = the library's draws (pgps_philox.h).
template <typename T>
int seq_sample(long N, int d, const T* Fs, const T* Qs, const T* fms, const T* fPs, int S, long s0, unsigned long long seed,
               const T* z, const T* H, T* out) {
    if (N < 1 || d < 1 || S < 1 || s0 < 0 || s0 + S > 0xffffffffL || !Fs || !Qs || !fms || !fPs || !out) return PGPS_E_INVALID;
    if (d > PGPS_MAX_DIM) return PGPS_E_UNSUPPORTED_DIM;
    const size_t dd = (size_t)d * d;
    Seq<T> w(d);
    std::vector<T> x((size_t)S * d), E(dd), g(d), L(dd), C(dd), Pp(dd), A(dd), X(dd), mp(d), zv(d + 1), t(d);
    for (long k = N - 1; k >= 0; --k) {
        const T* m = fms + k * d;
        const T* P = fPs + k * dd;
        if (k == N - 1) {
            for (size_t i = 0; i < dd; ++i) { E[i] = T(0); L[i] = T(0.5) * (P[i] + P[(i % d) * d + i / d]); }
            for (int i = 0; i < d; ++i) g[i] = m[i];
        } else {
            const T* F = Fs + (k + 1) * dd;
            w.predict(F, P, Qs + (k + 1) * dd, Pp.data());           // Pp; w.FP = F P
            for (size_t i = 0; i < dd; ++i) { A[i] = Pp[i]; X[i] = w.FP[i]; }
            if (!lu_solve(d, A.data(), X.data())) return PGPS_E_NUMERIC;         // X = Pp^-1 F P = E^T
            for (int i = 0; i < d; ++i)
                for (int j = 0; j < d; ++j) E[i * d + j] = X[j * d + i];
            for (int i = 0; i < d; ++i) {
                T acc = 0;
                for (int j = 0; j < d; ++j) acc += F[i * d + j] * m[j];
                mp[i] = acc;
            }
            for (int i = 0; i < d; ++i) {
                T acc = 0;
                for (int j = 0; j < d; ++j) acc += E[i * d + j] * mp[j];
                g[i] = m[i] - acc;
            }
            for (int i = 0; i < d; ++i)
                for (int j = 0; j < d; ++j) {
                    T a = 0, b = 0;
                    for (int l = 0; l < d; ++l) { a += E[i * d + l] * w.FP[l * d + j]; b += E[j * d + l] * w.FP[l * d + i]; }
                    L[i * d + j] = T(0.5) * (P[i * d + j] + P[j * d + i]) - T(0.5) * (a + b);
                }
        }
        T pmax = P[0];
        for (int i = 1; i < d; ++i) pmax = P[i * d + i] > pmax ? P[i * d + i] : pmax;
        psd_chol_rt(d, L.data(), pmax, C.data());
        for (int s = 0; s < S; ++s) {
            T* xs = x.data() + (size_t)s * d;
            if (z) {
                for (int i = 0; i < d; ++i) zv[i] = z[((size_t)s * N + k) * d + i];
            } else {
                for (int j = 0; j < (d + 1) / 2; ++j) pgps::normal_pair<T>(seed, k, (uint32_t)(s0 + s), (uint32_t)j, zv[2 * j], zv[2 * j + 1]);
            }
            for (int i = 0; i < d; ++i) {
                T acc = g[i];
                for (int j = 0; j < d; ++j) acc += E[i * d + j] * xs[j];
                for (int j = 0; j < d; ++j) acc += C[i * d + j] * zv[j];
                t[i] = acc;
            }
            for (int i = 0; i < d; ++i) xs[i] = t[i];
            if (H) {
                T acc = 0;
                for (int i = 0; i < d; ++i) acc += H[i] * xs[i];
                out[(size_t)s * N + k] = acc;
            } else {
                for (int i = 0; i < d; ++i) out[((size_t)s * N + k) * d + i] = xs[i];
            }
        }
    }
    return PGPS_OK;
}

// Joint covariance between selected steps, the definition of pgps_pks_cov_*: Cov(x_i, x_j | ys) =
// E_i .. E_{j-1} sP_j for i < j, E_k = P_k F_{k+1}^T Pp_{k+1}^-1 the gain of step k's smoothing element.  First the products
// B_a between consecutive selected steps, then column by column v <- B_{i-1} v from v = sym(sP_j) (H^T) upwards.
template <typename T>
int seq_cov(long N, int d, const T* Fs, const T* Qs, const T* fPs, const T* sPs, long n, const long* sel, const T* H, T* out) {
    if (N < 1 || d < 1 || n < 1 || n > N || !Fs || !Qs || !fPs || !sPs || !sel || !out) return PGPS_E_INVALID;
    if (d > PGPS_MAX_DIM) return PGPS_E_UNSUPPORTED_DIM;
    for (long a = 0; a < n; ++a)
        if (sel[a] < 0 || sel[a] >= N || (a > 0 && sel[a - 1] >= sel[a])) return PGPS_E_INVALID;
    const size_t dd = (size_t)d * d;
    Seq<T> w(d);
    std::vector<T> B((size_t)(n - 1) * dd), E(dd), Pp(dd), A(dd), X(dd), acc(dd), tmp(dd);
    for (long a = 0; a + 1 < n; ++a) {
        for (size_t i = 0; i < dd; ++i) acc[i] = T(0);
        for (int i = 0; i < d; ++i) acc[(size_t)i * d + i] = T(1);
        for (long k = sel[a]; k < sel[a + 1]; ++k) {
            w.predict(Fs + (k + 1) * dd, fPs + k * dd, Qs + (k + 1) * dd, Pp.data());      // Pp; w.FP = F P
            for (size_t i = 0; i < dd; ++i) { A[i] = Pp[i]; X[i] = w.FP[i]; }
            if (!lu_solve(d, A.data(), X.data())) return PGPS_E_NUMERIC;                    // X = Pp^-1 F P = E^T
            for (int i = 0; i < d; ++i)
                for (int j = 0; j < d; ++j) {
                    T s = 0;
                    for (int l = 0; l < d; ++l) s += acc[i * d + l] * X[j * d + l];
                    tmp[i * d + j] = s;
                }
            acc = tmp;
        }
        for (size_t i = 0; i < dd; ++i) B[(size_t)a * dd + i] = acc[i];
    }
    const int W = H ? 1 : d;
    std::vector<T> V((size_t)d * W), Vn((size_t)d * W);
    for (long j = 0; j < n; ++j) {
        const T* P = sPs + sel[j] * dd;
        for (int i = 0; i < d; ++i) {
            if (H) {
                T s = 0;
                for (int l = 0; l < d; ++l) s += T(0.5) * (P[i * d + l] + P[l * d + i]) * H[l];
                V[i] = s;
            } else {
                for (int l = 0; l < d; ++l) V[(size_t)i * d + l] = T(0.5) * (P[i * d + l] + P[l * d + i]);
            }
        }
        for (long i = j; i >= 0; --i) {
            if (H) {
                T c = 0;
                for (int l = 0; l < d; ++l) c += H[l] * V[l];
                out[(size_t)i * n + j] = c;
                out[(size_t)j * n + i] = c;
            } else {
                for (int p = 0; p < d; ++p)
                    for (int q = 0; q < d; ++q) {
                        out[((size_t)i * n + j) * dd + p * d + q] = V[(size_t)p * d + q];
                        out[((size_t)j * n + i) * dd + q * d + p] = V[(size_t)p * d + q];
                    }
            }
            if (i > 0) {
                const T* Bi = B.data() + (size_t)(i - 1) * dd;
                for (int p = 0; p < d; ++p)
                    for (int q = 0; q < W; ++q) {
                        T s = 0;
                        for (int l = 0; l < d; ++l) s += Bi[p * d + l] * V[(size_t)l * W + q];
                        Vn[(size_t)p * W + q] = s;
                    }
                V = Vn;
            }
        }
    }
    return PGPS_OK;
}

template <typename T>
int seq_normals(long N, int d, int S, long s0, unsigned long long seed, T* z) {
    if (N < 1 || d < 1 || S < 1 || s0 < 0 || s0 + S > 0xffffffffL || !z) return PGPS_E_INVALID;
    for (int s = 0; s < S; ++s)
        for (long k = 0; k < N; ++k)
            for (int j = 0; j < (d + 1) / 2; ++j) {
                T a, b;
                pgps::normal_pair<T>(seed, k, (uint32_t)(s0 + s), (uint32_t)j, a, b);
                T* o = z + ((size_t)s * N + k) * d;
                o[2 * j] = a;
                if (2 * j + 1 < d) o[2 * j + 1] = b;
            }
    return PGPS_OK;
}

}  // namespace

extern "C" int pgps_seq_kf_f64(long N, int d, const double* P0, const double* Fs, const double* Qs, const double* H,
                               double R, const double* ys, double* fms, double* fPs, double* ll, double* mps,
                               double* Pps) {
    return seq_kf<double>(N, d, P0, Fs, Qs, H, R, ys, fms, fPs, ll, mps, Pps);
}
extern "C" int pgps_seq_kf_f32(long N, int d, const float* P0, const float* Fs, const float* Qs, const float* H,
                               float R, const float* ys, float* fms, float* fPs, double* ll, float* mps, float* Pps) {
    return seq_kf<float>(N, d, P0, Fs, Qs, H, R, ys, fms, fPs, ll, mps, Pps);
}
extern "C" int pgps_seq_kf_het_f64(long N, int d, const double* P0, const double* Fs, const double* Qs, const double* H,
                                   const double* Rs, const double* ys, double* fms, double* fPs, double* ll, double* mps,
                                   double* Pps) {
    if (!Rs) return PGPS_E_INVALID;
    return seq_kf<double>(N, d, P0, Fs, Qs, H, 0.0, ys, fms, fPs, ll, mps, Pps, Rs);
}
extern "C" int pgps_seq_kf_het_f32(long N, int d, const float* P0, const float* Fs, const float* Qs, const float* H,
                                   const float* Rs, const float* ys, float* fms, float* fPs, double* ll, float* mps, float* Pps) {
    if (!Rs) return PGPS_E_INVALID;
    return seq_kf<float>(N, d, P0, Fs, Qs, H, 0.0f, ys, fms, fPs, ll, mps, Pps, Rs);
}
extern "C" int pgps_seq_ks_f64(long N, int d, const double* Fs, const double* ms, const double* Ps, const double* mps,
                               const double* Pps, double* sms, double* sPs) {
    return seq_ks<double>(N, d, Fs, ms, Ps, mps, Pps, sms, sPs);
}
extern "C" int pgps_seq_ks_f32(long N, int d, const float* Fs, const float* ms, const float* Ps, const float* mps,
                               const float* Pps, float* sms, float* sPs) {
    return seq_ks<float>(N, d, Fs, ms, Ps, mps, Pps, sms, sPs);
}

// The sweep of balance_ss (pssgp/kernels/math_utils.py:10-29, a numba loop in the reference): n_iter passes over the
// states, each visit equalising the off-diagonal column and row 2-norms of the progressively rescaled matrix; returns
// the accumulated diagonal scaling.  It is the inner loop of every get_sde() of a composite kernel, i.e. of every
// hyper-parameter setting an optimiser or sampler visits.  0/0 (an isolated state) gives NaN, as in the reference.
extern "C" int pgps_host_balance_f64(int d, const double* F, int n_iter, double* scale) {
    if (d < 1 || !F || !scale || n_iter < 0) return PGPS_E_INVALID;
    std::vector<double> W((size_t)d * d);
    for (int i = 0; i < d; ++i)
        for (int j = 0; j < d; ++j) W[(size_t)i * d + j] = (i == j) ? 0.0 : F[(size_t)i * d + j];
    for (int i = 0; i < d; ++i) scale[i] = 1.0;
    for (int it = 0; it < n_iter; ++it)
        for (int i = 0; i < d; ++i) {
            double c = 0.0, r = 0.0;
            for (int k = 0; k < d; ++k) {
                c += W[(size_t)k * d + i] * W[(size_t)k * d + i];
                r += W[(size_t)i * d + k] * W[(size_t)i * d + k];
            }
            const double f = std::pow(r / c, 0.25);
            scale[i] *= f;
            for (int k = 0; k < d; ++k) {
                W[(size_t)k * d + i] *= f;
                W[(size_t)i * d + k] /= f;
            }
        }
    return PGPS_OK;
}

extern "C" int pgps_seq_ks_sample_f64(long N, int d, const double* Fs, const double* Qs, const double* fms, const double* fPs,
                                      int S, long s0, unsigned long long seed, const double* z, const double* H, double* out) {
    return seq_sample<double>(N, d, Fs, Qs, fms, fPs, S, s0, seed, z, H, out);
}
extern "C" int pgps_seq_ks_sample_f32(long N, int d, const float* Fs, const float* Qs, const float* fms, const float* fPs,
                                      int S, long s0, unsigned long long seed, const float* z, const float* H, float* out) {
    return seq_sample<float>(N, d, Fs, Qs, fms, fPs, S, s0, seed, z, H, out);
}
extern "C" int pgps_seq_sample_normals_f64(long N, int d, int S, long s0, unsigned long long seed, double* z) {
    return seq_normals<double>(N, d, S, s0, seed, z);
}
extern "C" int pgps_seq_sample_normals_f32(long N, int d, int S, long s0, unsigned long long seed, float* z) {
    return seq_normals<float>(N, d, S, s0, seed, z);
}
extern "C" int pgps_seq_ks_cov_f64(long N, int d, const double* Fs, const double* Qs, const double* fPs, const double* sPs,
                                   long n, const long* sel, const double* H, double* out) {
    return seq_cov<double>(N, d, Fs, Qs, fPs, sPs, n, sel, H, out);
}
extern "C" int pgps_seq_ks_cov_f32(long N, int d, const float* Fs, const float* Qs, const float* fPs, const float* sPs, long n,
                                   const long* sel, const float* H, float* out) {
    return seq_cov<float>(N, d, Fs, Qs, fPs, sPs, n, sel, H, out);
}
