// interpolator.hpp -- AMG::InterpolatorBase / AMG::LinearInterpolator of the drop-in.
//
// Same public interface as the reference's interpolator.hpp (constructors, the pure
// virtual make_operators(n_h, n_H, level), prolongation / restriction, the P / R getters
// and setters); the products run on the device through the C ABI.  Inside the V-cycle
// the operators of LinearInterpolator are recognised and replaced by matrix-free kernels.
#pragma once
#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include <amg/eigen_lite.hpp>

namespace AMG {

template <class EleType>
class InterpolatorBase {
  using Sparse = Eigen::SparseMatrix<EleType>;
  using Vector = Eigen::Matrix<EleType, -1, 1>;

  std::vector<Sparse> prolong_;   // level l -> P_l (fine x coarse)
  std::vector<Sparse> restrict_;  // level l -> R_l (coarse x fine)

  // M * v as one device SpMV (interpolator.hpp:52-56 and :64-68 of the reference)
  static Vector device_product(const Sparse& M, const Vector& v) {
    static_assert(sizeof(EleType) == sizeof(double), "the MI355X path is fp64 only");
    const Sparse packed = detail::compressed(M);
    Vector out(packed.rows());
    detail::check(amg_hip_spmv(packed.rows(), packed.cols(), packed.outerIndexPtr(),
                               packed.innerIndexPtr(), packed.valuePtr(), v.data(), out.data()));
    return out;
  }

 public:
  InterpolatorBase() = default;
  InterpolatorBase(size_t n_levels) : prolong_(n_levels - 1), restrict_(n_levels - 1) {}
  virtual ~InterpolatorBase() = default;

  // fills P and R of `level` for a fine level of n_h_dofs and a coarse one of n_H_dofs
  virtual void make_operators(size_t n_h_dofs, size_t n_H_dofs, size_t level) = 0;

  Vector prolongation(const Vector& v, size_t level) { return device_product(prolong_[level], v); }
  Vector restriction(const Vector& v, size_t level) { return device_product(restrict_[level], v); }

  const Sparse& get_P(size_t level) const { return prolong_[level]; }
  const Sparse& get_R(size_t level) const { return restrict_[level]; }
  // (an interpolator constructed without a level count grows on demand)
  void set_level_to_P(size_t level, Sparse& P) {
    if (level >= prolong_.size()) prolong_.resize(level + 1);
    prolong_[level] = P;
  }
  void set_level_to_R(size_t level, Sparse& R) {
    if (level >= restrict_.size()) restrict_.resize(level + 1);
    restrict_[level] = R;
  }
  size_t n_operator_levels() const { return prolong_.size(); }
};

// 1-D linear interpolation in the flat index: coarse dof c feeds fine rows 2c, 2c+1, 2c+2
// with weights 1/2, 1, 1/2 (rows past the fine level are dropped); R is P transposed.
template <class EleType>
class LinearInterpolator : public InterpolatorBase<EleType> {
 public:
  using InterpolatorBase<EleType>::InterpolatorBase;

  void make_operators(size_t n_h_dofs, size_t n_H_dofs, size_t level) override {
    static const std::array<EleType, 3> weight = {EleType(0.5), EleType(1.0), EleType(0.5)};
    std::vector<Eigen::Triplet<EleType>> entries;
    entries.reserve(weight.size() * n_H_dofs);
    for (size_t coarse = 0; coarse < n_H_dofs; ++coarse)
      for (size_t k = 0; k < weight.size(); ++k) {
        const size_t fine = 2 * coarse + k;
        if (fine < n_h_dofs) entries.emplace_back(fine, coarse, weight[k]);
      }
    Eigen::SparseMatrix<EleType> P(n_h_dofs, n_H_dofs);
    P.setFromTriplets(entries.begin(), entries.end());
    Eigen::SparseMatrix<EleType> R = P.transpose();
    this->set_level_to_P(level, P);
    this->set_level_to_R(level, R);
  }
};

// Strength-based C/F coarsening with direct interpolation -- the alternative the reference's
// README.md:104-109 names and does not build (NO reference counterpart).  Its operators depend
// on the level MATRIX, which make_operators(n_h, n_H, level) is never told, so AMG::Multigrid
// recognises the class and lets the library build the hierarchy (amg_hip_create_rs): `n_levels`
// is then an upper bound, Multigrid::get_n_levels() tells how many were built, and get_P /
// get_R hold the operators afterwards.
template <class EleType>
class RugeStuebenInterpolator : public InterpolatorBase<EleType> {
  EleType theta_;
  size_t min_coarse_;

 public:
  explicit RugeStuebenInterpolator(size_t max_levels, EleType theta = 0.25, size_t min_coarse = 500)
      : InterpolatorBase<EleType>(max_levels), theta_(theta), min_coarse_(min_coarse) {}
  EleType theta() const { return theta_; }
  size_t min_coarse() const { return min_coarse_; }
  void make_operators(size_t, size_t, size_t) override {
    throw std::logic_error("RugeStuebenInterpolator: the operators depend on the level matrix; "
                           "AMG::Multigrid builds them");
  }
};

// Full coarsening of an nx x ny (x nz) grid, x fastest (dof = (k ny + j) nx + i): the 1-D rule of
// LinearInterpolator applied per axis -- NO reference counterpart (the reference halves the flat
// index, which coarsens x only).  Every axis of length m goes to floor(m / 2) (nz = 1: a 2-D grid,
// z is left alone), P = P1(nz) (x) P1(ny) (x) P1(nx) with P1(m) the m x floor(m / 2) matrix holding
// 1/2, 1, 1/2 on rows 2j, 2j+1, 2j+2 (< m) of column j, R = P^T.  The level sizes differ from the
// reference's (n + 1) / 2 - 1, so AMG::Multigrid recognises the class and lets the library build
// the hierarchy (amg_hip_create_tensor: the matrix-free transfer kernels); get_P / get_R hold the
// operators afterwards, and make_operators gives exactly those for a caller that wants them alone.
template <class EleType>
class TensorInterpolator : public InterpolatorBase<EleType> {
  std::array<size_t, 3> dims_;
  bool three_d_;

 public:
  TensorInterpolator(size_t nx, size_t ny, size_t nz = 1) : dims_{nx, ny, nz}, three_d_(nz > 1) {
    if (nx < 1 || ny < 1 || nz < 1) throw std::invalid_argument("TensorInterpolator: empty grid");
  }
  int dim() const { return three_d_ ? 3 : 2; }
  std::array<size_t, 3> dims() const { return dims_; }
  // grid of `level` (level 0 = the constructor's)
  std::array<size_t, 3> level_dims(size_t level) const {
    std::array<size_t, 3> d = dims_;
    for (size_t l = 0; l < level; ++l) {
      d[0] /= 2;
      d[1] /= 2;
      if (three_d_) d[2] /= 2;
    }
    return d;
  }

  void make_operators(size_t n_h_dofs, size_t n_H_dofs, size_t level) override {
    static const std::array<EleType, 3> weight = {EleType(0.5), EleType(1.0), EleType(0.5)};
    const std::array<size_t, 3> d = level_dims(level), c = level_dims(level + 1);
    if (d[0] * d[1] * d[2] != n_h_dofs || c[0] * c[1] * c[2] != n_H_dofs || n_H_dofs < 1)
      throw std::invalid_argument("TensorInterpolator: level " + std::to_string(level) + " is a " +
                                  std::to_string(d[0]) + " x " + std::to_string(d[1]) + " x " +
                                  std::to_string(d[2]) + " grid, its coarse level has " +
                                  std::to_string(c[0] * c[1] * c[2]) + " dofs");
    const size_t tz_n = three_d_ ? 3 : 1;
    std::vector<Eigen::Triplet<EleType>> entries;
    entries.reserve((three_d_ ? 27 : 9) * n_H_dofs);
    for (size_t K = 0; K < c[2]; ++K)
      for (size_t J = 0; J < c[1]; ++J)
        for (size_t I = 0; I < c[0]; ++I) {
          const size_t coarse = (K * c[1] + J) * c[0] + I;
          for (size_t tz = 0; tz < tz_n; ++tz) {
            const size_t k = three_d_ ? 2 * K + tz : 0;
            if (k >= d[2]) continue;
            const EleType wz = three_d_ ? weight[tz] : EleType(1.0);
            for (size_t ty = 0; ty < 3; ++ty) {
              const size_t j = 2 * J + ty;
              if (j >= d[1]) continue;
              for (size_t tx = 0; tx < 3; ++tx) {
                const size_t i = 2 * I + tx;
                if (i >= d[0]) continue;
                entries.emplace_back((k * d[1] + j) * d[0] + i, coarse, wz * weight[ty] * weight[tx]);
              }
            }
          }
        }
    Eigen::SparseMatrix<EleType> P(n_h_dofs, n_H_dofs);
    P.setFromTriplets(entries.begin(), entries.end());
    Eigen::SparseMatrix<EleType> R = P.transpose();
    this->set_level_to_P(level, P);
    this->set_level_to_R(level, R);
  }
};

// Semi-coarsening of the same grids (amg_hip_create_tensor_semi; NO reference counterpart): level l
// coarsens the axes of its mask (bit 0 = x, 1 = y, 2 = z) with P1 and leaves the others alone
// (identity).  `masks` empty: the library's automatic rule -- the axes whose strongest pure-axis
// coupling is at least theta times the strongest of all, until n_levels, a level of at most
// min_coarse rows or a grid without an axis of 2 points (Multigrid::get_n_levels tells).  The
// operators depend on the level matrices, so AMG::Multigrid lets the library build the hierarchy;
// get_P / get_R hold the operators afterwards.  For operators that are anisotropic along a grid
// axis, where full coarsening with a point smoother stalls.
template <class EleType>
class SemiTensorInterpolator : public TensorInterpolator<EleType> {
  std::vector<int32_t> masks_;
  double theta_;
  size_t min_coarse_;

 public:
  SemiTensorInterpolator(size_t nx, size_t ny, size_t nz = 1, std::vector<int32_t> masks = {},
                         double theta = 0.5, size_t min_coarse = 32)
      : TensorInterpolator<EleType>(nx, ny, nz), masks_(std::move(masks)), theta_(theta), min_coarse_(min_coarse) {}
  const std::vector<int32_t>& masks() const { return masks_; }
  double theta() const { return theta_; }
  size_t min_coarse() const { return min_coarse_; }
  void make_operators(size_t, size_t, size_t) override {
    throw std::logic_error("SemiTensorInterpolator: the coarsened axes depend on the level matrix; "
                           "AMG::Multigrid builds the operators");
  }
};

// Operator-dependent interpolation on the same grids (amg_hip_create_tensor_opdep; NO reference
// counterpart): every level coarsens exactly ONE axis (masks of one bit: 1 = x, 2 = y, 4 = z), and the
// 1-D weights along it come from the rows of the level's own matrix, collapsed onto that axis.
// `masks` empty: the library's automatic rule -- the axis with the strongest pure-axis coupling, the
// lowest on a tie, until n_levels, a level of at most min_coarse rows or a grid without an axis of 2
// points (Multigrid::get_n_levels tells).  AMG::Multigrid lets the library build the hierarchy;
// get_P / get_R hold the operators afterwards.  For coefficients that jump by orders of magnitude
// from cell to cell, where fixed weights leave the smooth error to the Krylov method.
// periodic_axes (bit a = axis a, default 0): the axes that wrap (amg_hip_create_tensor_opdep_periodic):
// A holds the wrap entries, a coarsened periodic axis needs an even length of at least 4, and fine
// point 0 of such an axis takes its low weight from the last coarse point.
template <class EleType>
class OpdepTensorInterpolator : public TensorInterpolator<EleType> {
  std::vector<int32_t> masks_;
  size_t min_coarse_;
  int32_t periodic_axes_;

 public:
  OpdepTensorInterpolator(size_t nx, size_t ny, size_t nz = 1, std::vector<int32_t> masks = {},
                          size_t min_coarse = 32, int32_t periodic_axes = 0)
      : TensorInterpolator<EleType>(nx, ny, nz), masks_(std::move(masks)), min_coarse_(min_coarse),
        periodic_axes_(periodic_axes) {}
  const std::vector<int32_t>& masks() const { return masks_; }
  size_t min_coarse() const { return min_coarse_; }
  int32_t periodic_axes() const { return periodic_axes_; }
  void make_operators(size_t, size_t, size_t) override {
    throw std::logic_error("OpdepTensorInterpolator: the weights depend on the level matrix; "
                           "AMG::Multigrid builds the operators");
  }
};

}  // namespace AMG
