// Drop-in for include/amg/smoother.hpp: same classes, same constructors, same
// public fields; smooth() runs on the GPU through amg_hip.h.
#pragma once
#include <iostream>
#include <stdexcept>
#include <string>

#include <amg/common.hpp>

namespace AMG {

// reference smoother.hpp:18-66
template <class EleType>
class SmootherBase {
 public:
  EleType tolerance{1e-9};
  size_t compute_error_every_n_iters{100};
  size_t n_iters{1};

  SmootherBase() {}
  SmootherBase(size_t n_iters_) : n_iters(n_iters_) {}
  SmootherBase(double tolerance_, size_t compute_error_every_n_iters_, size_t n_iters_)
      : tolerance(tolerance_), compute_error_every_n_iters(compute_error_every_n_iters_),
        n_iters(n_iters_) {}
  virtual ~SmootherBase() {}

  virtual void smooth(const Eigen::SparseMatrix<EleType>& A, Eigen::Matrix<EleType, -1, 1>& u,
                      const Eigen::Matrix<EleType, -1, 1>& b) = 0;
};

namespace detail {
template <class EleType>
inline void device_smooth(int kind, const Eigen::SparseMatrix<EleType>& A,
                          Eigen::Matrix<EleType, -1, 1>& u, const Eigen::Matrix<EleType, -1, 1>& b,
                          double omega, double tol, size_t every, size_t n_iters, int64_t* iters,
                          int32_t* converged) {
  static_assert(sizeof(EleType) == sizeof(double), "the MI355X path is fp64 only");
  const Eigen::SparseMatrix<EleType> C = compressed(A);
  check(amg_hip_smooth(kind, C.rows(), C.outerIndexPtr(), C.innerIndexPtr(), C.valuePtr(),
                       u.data(), b.data(), omega, tol, (int64_t)every, (int64_t)n_iters, iters,
                       converged));
}
}  // namespace detail

// reference smoother.hpp:86-216: symmetric (forward + backward) lexicographic
// Gauss-Seidel, executed on the device in exact sequential order.
template <class EleType>
class SparseGaussSeidel : public SmootherBase<EleType> {
 public:
  using SmootherBase<EleType>::SmootherBase;
  SparseGaussSeidel() {  // smoother.hpp:183-187
    this->tolerance = 1e-9;
    this->compute_error_every_n_iters = 0;
    this->n_iters = 1;
  }
  void smooth(const Eigen::SparseMatrix<EleType>& A, Eigen::Matrix<EleType, -1, 1>& u,
              const Eigen::Matrix<EleType, -1, 1>& b) override {
    int64_t iter = 0;
    int32_t conv = 0;
    detail::device_smooth(AMG_HIP_SM_SPGS, A, u, b, 1.0, this->tolerance,
                          this->compute_error_every_n_iters, this->n_iters, &iter, &conv);
    if (this->compute_error_every_n_iters != 0) {  // smoother.hpp:205-212
      if (conv) std::cout << "SPGS converged after " << iter << " iterations." << std::endl;
      else std::cout << "SPGS did not converge after " << iter << " iterations." << std::endl;
    }
  }
};

// reference smoother.hpp:223-264 (an in-place forward Gauss-Seidel)
template <class EleType>
class Jacobi : public SmootherBase<EleType> {
 public:
  using SmootherBase<EleType>::SmootherBase;
  Jacobi() {}
  void smooth(const Eigen::SparseMatrix<EleType>& A, Eigen::Matrix<EleType, -1, 1>& u,
              const Eigen::Matrix<EleType, -1, 1>& b) override {
    detail::device_smooth(AMG_HIP_SM_REF_JACOBI, A, u, b, 1.0, this->tolerance,
                          this->compute_error_every_n_iters, this->n_iters, nullptr, nullptr);
  }
};

// reference smoother.hpp:271-373
template <class EleType>
class SuccessiveOverRelaxation : public SmootherBase<EleType> {
  double omega{1.0};
  void validate_omega() {  // smoother.hpp:286-293
    if (omega > 2 || omega < 0) {
      std::string msg = "`omega` must be in [0, 2] but got omega=" + std::to_string(omega) + "\n";
      throw std::invalid_argument(msg);
    }
  }

 public:
  using SmootherBase<EleType>::SmootherBase;
  SuccessiveOverRelaxation() {}
  SuccessiveOverRelaxation(double omega_) : omega(omega_) { validate_omega(); }
  SuccessiveOverRelaxation(double omega_, double tolerance_, size_t compute_error_every_n_iters_,
                           size_t n_iters_)
      : SmootherBase<EleType>(tolerance_, compute_error_every_n_iters_, n_iters_), omega(omega_) {
    validate_omega();
  }
  double get_omega() const { return omega; }
  void smooth(const Eigen::SparseMatrix<EleType>& A, Eigen::Matrix<EleType, -1, 1>& u,
              const Eigen::Matrix<EleType, -1, 1>& b) override {
    detail::device_smooth(AMG_HIP_SM_SOR, A, u, b, omega, this->tolerance,
                          this->compute_error_every_n_iters, this->n_iters, nullptr, nullptr);
  }
};

// Build-side addition (no reference counterpart): true two-buffer weighted Jacobi,
// u <- u + omega*(D^-1 (b - (A-D) u) - u), `n_iters` sweeps per smooth().  Fully
// parallel: this is the throughput smoother of the MI355X path.  omega must stay
// below 2/lambda_max(D^-1 A) (~0.67 on the reference's coarse Galerkin levels).
template <class EleType>
class TrueJacobi : public SmootherBase<EleType> {
  double omega{0.6};

 public:
  TrueJacobi() { this->n_iters = 2; this->compute_error_every_n_iters = 0; }
  TrueJacobi(double omega_, size_t n_sweeps = 2) : omega(omega_) {
    this->n_iters = n_sweeps;
    this->compute_error_every_n_iters = 0;
  }
  double get_omega() const { return omega; }
  void smooth(const Eigen::SparseMatrix<EleType>& A, Eigen::Matrix<EleType, -1, 1>& u,
              const Eigen::Matrix<EleType, -1, 1>& b) override {
    detail::device_smooth(AMG_HIP_SM_JACOBI, A, u, b, omega, 0.0, 0, this->n_iters, nullptr, nullptr);
  }
};

// Build-side addition (no reference counterpart): Chebyshev polynomial smoother in D^-1 A of degree
// `degree` on [lower G, upper G], G = max_i (sum_j |a_ij|) / |a_ii| (Gershgorin); `n_iters`
// applications per smooth(), each `degree` fully parallel Jacobi-shaped passes.  A polynomial in
// D^-1 A: the same pre- and post-smoother keep the V-cycle symmetric (AMG::PCG).  No colouring, no
// omega to tune (amg_hip.h: AMG_HIP_SM_CHEBYSHEV).
template <class EleType>
class Chebyshev : public SmootherBase<EleType> {
  int degree{2};
  double lower{0.3}, upper{1.0};

 public:
  Chebyshev(int degree_ = 2, double lower_ = 0.3, double upper_ = 1.0, size_t n_iters_ = 1)
      : degree(degree_), lower(lower_), upper(upper_) {
    this->n_iters = n_iters_;
    this->compute_error_every_n_iters = 0;
    if (degree < 1) throw std::invalid_argument("`degree` must be at least 1");
    if (!(lower > 0.0) || !(lower < upper))
      throw std::invalid_argument("the interval must satisfy 0 < lower < upper");
  }
  int get_degree() const { return degree; }
  double get_lower() const { return lower; }
  double get_upper() const { return upper; }
  void smooth(const Eigen::SparseMatrix<EleType>& A, Eigen::Matrix<EleType, -1, 1>& u,
              const Eigen::Matrix<EleType, -1, 1>& b) override {
    static_assert(sizeof(EleType) == sizeof(double), "the MI355X path is fp64 only");
    const Eigen::SparseMatrix<EleType> C = detail::compressed(A);
    detail::check(amg_hip_smooth_chebyshev(C.rows(), C.outerIndexPtr(), C.innerIndexPtr(), C.valuePtr(),
                                           u.data(), b.data(), degree, lower, upper, (int64_t)this->n_iters));
  }
};

// Build-side addition (no reference counterpart): line relaxation, Jacobi between the lines
// (amg_hip.h: AMG_HIP_SM_LINE_JACOBI).  One sweep is u <- u + omega T^-1 (b - A u), T the
// tridiagonal part of A along the lines the level's stride rule picks; `n_iters` sweeps per smooth().
// On the hierarchies that halve the flat index it relaxes the lines of the direction that is not
// coarsened.  omega in (0, 2); 0.7 is the recommended value (1.0 converges poorly).
template <class EleType>
class LineJacobi : public SmootherBase<EleType> {
  double omega{0.7};

 public:
  LineJacobi(double omega_ = 0.7, size_t n_iters_ = 1) : omega(omega_) {
    this->n_iters = n_iters_;
    this->compute_error_every_n_iters = 0;
    if (!(omega > 0.0 && omega < 2.0)) throw std::invalid_argument("`omega` must lie in (0, 2)");
  }
  double get_omega() const { return omega; }
  void smooth(const Eigen::SparseMatrix<EleType>& A, Eigen::Matrix<EleType, -1, 1>& u,
              const Eigen::Matrix<EleType, -1, 1>& b) override {
    static_assert(sizeof(EleType) == sizeof(double), "the MI355X path is fp64 only");
    const Eigen::SparseMatrix<EleType> C = detail::compressed(A);
    detail::check(amg_hip_smooth_line(C.rows(), C.outerIndexPtr(), C.innerIndexPtr(), C.valuePtr(), 0, omega,
                                      (int64_t)this->n_iters, u.data(), b.data()));
  }
};

// Build-side addition (no reference counterpart): alternating-direction line relaxation on the
// nx x ny (x nz) grid of a full-coarsening hierarchy (amg_hip.h: AMG_HIP_SM_LINE_ALT).  One
// application is one sub-sweep u <- u + omega T_a^-1 (b - A u) per axis of length >= 2, x first;
// inside a Multigrid built with a TensorInterpolator every level uses its own grid and the up-leg
// runs the axes in descending order (any other interpolator is refused).  smooth() is the
// stand-alone ascending application on the grid given here.  omega in (0, 2); 0.8 is recommended.
template <class EleType>
class LineAlternating : public SmootherBase<EleType> {
  double omega{0.8};
  int dim_{2};
  int64_t dims_[3]{1, 1, 1};

 public:
  LineAlternating(size_t nx, size_t ny, double omega_ = 0.8, size_t n_iters_ = 1) : omega(omega_) {
    init(2, nx, ny, 1, n_iters_);
  }
  LineAlternating(size_t nx, size_t ny, size_t nz, double omega_, size_t n_iters_) : omega(omega_) {
    init(3, nx, ny, nz, n_iters_);
  }
  double get_omega() const { return omega; }
  void smooth(const Eigen::SparseMatrix<EleType>& A, Eigen::Matrix<EleType, -1, 1>& u,
              const Eigen::Matrix<EleType, -1, 1>& b) override {
    static_assert(sizeof(EleType) == sizeof(double), "the MI355X path is fp64 only");
    const Eigen::SparseMatrix<EleType> C = detail::compressed(A);
    detail::check(amg_hip_smooth_line_alt(C.rows(), C.outerIndexPtr(), C.innerIndexPtr(), C.valuePtr(), dim_, dims_,
                                          omega, (int64_t)this->n_iters, 0, u.data(), b.data()));
  }

 private:
  void init(int dim, size_t nx, size_t ny, size_t nz, size_t n_iters_) {
    dim_ = dim;
    dims_[0] = (int64_t)nx;
    dims_[1] = (int64_t)ny;
    dims_[2] = (int64_t)nz;
    this->n_iters = n_iters_;
    this->compute_error_every_n_iters = 0;
    if (!(omega > 0.0 && omega < 2.0)) throw std::invalid_argument("`omega` must lie in (0, 2)");
  }
};

}  // namespace AMG
