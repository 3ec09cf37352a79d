// =============================================================================
// kernels.hip -- hand-written gfx950 (CDNA4, wave64) kernels of the V-cycle.
//
// All kernels are HBM-bandwidth bound sparse fp64 kernels (~0.17 flop/byte):
// no MFMA.  Compile with -ffp-contract=off: parity with the reference's
// arithmetic (separate IEEE multiply/add, true divide) is part of
// the contract and several kernels are bit-exact against the CPU oracle.
//
// K-Dict (dict_kernel, dict_resid_restrict_kernel, dict_jacobi_prolong_kernel,
//   dict_gs_color_kernel)   -- residual / true Jacobi / SpMV / rss terms / one colour of
//   the multicolour GS on dictionary-coded matrices: 8 or 16 bytes of byte codes per
//   row into an LDS table of the matrix's distinct (column offset, value) pairs, and
//   the forms fused across a level boundary (residual + restriction + first coarse
//   sweep; last sweep + prolongation).  The default layout wherever a matrix qualifies.
// K-SELL (sell_kernel)      -- the same operations on CSR sliced into 64-row
//   lane-interleaved panels, 16-bit relative column indices, non-temporal matrix
//   stream (see the comment at the kernel).  Fallback layout; the fastest plain-CSR
//   form measured.
// K-CSR (csr_stage_kernel)  -- the same operations on plain CSR arrays (device-pointer
//   API, custom interpolators, fallback when SELL would pad too much).
//   One 256-thread workgroup owns 256 consecutive rows.  The workgroup's slice
//   of the CSR column-index and value arrays is contiguous in HBM, so it is
//   streamed with 16-byte-per-lane coalesced loads into LDS (the per-row
//   non-zeros are staged, never gathered).  Then one lane per row walks its
//   entries out of LDS in ascending column order (bit-exact summation order of
//   Eigen's column-major SpMV, multigrid.hpp:272-274) and gathers x[col]; for
//   banded stencil matrices consecutive lanes gather consecutive x, i.e. the
//   gathers coalesce into a few 128-B lines served by L1/L2.  LDS strides of 5
//   or 9 entries per lane are bank-conflict free for ds_read_b64 / ds_read_b32.
// K-Restrict / K-ProlongAdd -- matrix-free LinearInterpolator transfers.
// K-SumSq                   -- wave-shuffle + LDS tree reduction (deterministic).
// K-GS-lex (gs_lex_window)  -- exact lexicographic Gauss-Seidel, dependency
//   scheduled (parity mode, latency bound by construction).
// K-Band   (band_solve)     -- coarsest-level banded LDL^T solve, one wave.
// K-Spike  (spike_*)        -- the same solve partitioned over many waves (opt-in).
// K-Galerkin (galerkin_*)   -- setup: R (A P) for the linear interpolation pair.
// K-Halo / K-Gather         -- multi-GPU neighbour exchange and all-gather as
//   graph-capturable kernels over hipIpc-mapped peer memory.
// K-F32 (sell_f32_kernel, csr_f32_kernel, to_f32 / to_f64) -- the row kernels and transfers in
//   float for the single-precision preconditioner of the fp64 PCG.
// K-DictF32 (dict_f32_kernel) -- K-Dict's plain row path on float vectors: the double matrix's codes,
//   row types and offsets, a float copy of the pair table's values.
// =============================================================================
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <stdint.h>

#include <cstdio>
#include <type_traits>
#include <utility>
#include <vector>
#include <algorithm>
#include <cmath>

#include "kernels.hpp"

namespace amg_hip {

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also waits for every
// outstanding GLOBAL access of the wave (s_waitcnt vmcnt(0): prefetched operands, streamed-out
// results); kernels whose waves talk to each other through LDS alone use this one and keep
// their global loads and stores in flight across the barrier.
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// Chebyshev steps (kernels.hpp: CSR_CHEB, cheb_kernel_mode): template MODE 16 + first + 2 last.  The
// row walk is CSR_JACOBI's unchanged (same products, same order, same division); only the epilogue
// differs, so the results are bit-identical across layouts as the Jacobi sweeps are.
constexpr bool mode_cheb(int m) { return (m & ~3) == 16; }
constexpr bool mode_jac(int m) { return m == CSR_JACOBI || mode_cheb(m); }
constexpr bool cheb_first(int m) { return (m & 1) != 0; }
constexpr bool cheb_last(int m) { return (m & 2) != 0; }
// t = the Jacobi quotient t_i; z = t - x, d = alpha d + beta z (first step: beta z, d not read),
// out = x + d.  A first step is CSR_JACOBI's x + omega (t - x) with omega = beta, operation for operation.
template <int MODE>
__device__ __forceinline__ double cheb_update(double t, double xi, double di, double alpha, double beta,
                                              double& dn) {
  const double z = t - xi;
  dn = cheb_first(MODE) ? beta * z : alpha * di + beta * z;
  return xi + dn;
}

// ------------------------------------------------------------------ K-CSR ----
constexpr int CSR_BLOCK = 256;

template <int MODE, int K, int U>
__global__ __launch_bounds__(CSR_BLOCK) void csr_stage_kernel(
    int64_t n, int64_t nnz, const int32_t* __restrict__ rowptr,
    const int32_t* __restrict__ col, const double* __restrict__ val,
    const double* __restrict__ x, const double* f,  // f may be out (CSR_SPMV_ADD in place)
    double* out, double omega, int64_t diag_shift, double* dvec, double alpha) {
  constexpr int CAP = CSR_BLOCK * K;  // entries staged per chunk
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* lds_val = reinterpret_cast<double*>(smem);                    // CAP + 4
  int32_t* lds_col = reinterpret_cast<int32_t*>(smem + (CAP + 4) * 8);  // CAP + 4

  const int tid = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * CSR_BLOCK;
  const int64_t row = r0 + tid;
  const bool live = row < n;
  const int64_t rlast = (r0 + CSR_BLOCK < n) ? r0 + CSR_BLOCK : n;
  const int64_t p0 = rowptr[r0];
  const int64_t p1 = rowptr[rlast];
  int64_t rs = 0, re = 0;
  double fi = 0.0, xi = 0.0, di = 0.0;
  if (live) {
    rs = rowptr[row];
    re = rowptr[row + 1];
    if (MODE != CSR_SPMV) fi = f[row];
    if (mode_jac(MODE)) xi = x[row + diag_shift];
    if (mode_cheb(MODE) && !cheb_first(MODE)) di = dvec[row];
  }
  double acc = (MODE == CSR_RESID) ? fi : 0.0;
  double diag = 0.0;
  const int64_t drow = row + diag_shift;

  for (int64_t c0 = p0 & ~(int64_t)3; c0 < p1; c0 += CAP) {
    const int64_t c1 = (c0 + CAP < p1) ? c0 + CAP : p1;  // chunk = [c0, c1)
    const int cnt = (int)(c1 - c0);
    // ---- stage: coalesced 16-B loads HBM -> LDS ----
#pragma unroll
    for (int it = 0; it < K / 4 + 1; ++it) {
      const int i = (it * CSR_BLOCK + tid) * 4;
      if (i < cnt) {
        if (c0 + i + 4 <= nnz) {
          const int4 cc = *reinterpret_cast<const int4*>(col + c0 + i);
          *reinterpret_cast<int4*>(lds_col + i) = cc;
        } else {
          for (int t = 0; t < 4 && c0 + i + t < nnz; ++t) lds_col[i + t] = col[c0 + i + t];
        }
      }
    }
#pragma unroll
    for (int it = 0; it < K / 2 + 1; ++it) {
      const int i = (it * CSR_BLOCK + tid) * 2;
      if (i < cnt) {
        if (c0 + i + 2 <= nnz) {
          const double2 vv = *reinterpret_cast<const double2*>(val + c0 + i);
          *reinterpret_cast<double2*>(lds_val + i) = vv;
        } else {
          lds_val[i] = val[c0 + i];
        }
      }
    }
    __syncthreads();
    // ---- one lane per row, ascending column order ----
    int64_t p = rs > c0 ? rs : c0;
    const int64_t pe = re < c1 ? re : c1;
    while (p < pe) {
      int32_t c[U];
      double v[U], xx[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const bool ok = p + u < pe;
        const int o = ok ? (int)(p + u - c0) : (int)(p - c0);
        c[u] = lds_col[o];
        v[u] = lds_val[o];
      }
#pragma unroll
      for (int u = 0; u < U; ++u) xx[u] = x[c[u]];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (p + u < pe) {
          if (MODE == CSR_RESID) {
            acc -= v[u] * xx[u];
          } else if (mode_jac(MODE)) {
            if ((int64_t)c[u] == drow) diag = v[u];
            else acc += v[u] * xx[u];
          } else {
            acc += v[u] * xx[u];
          }
        }
      }
      p += U;
    }
    __syncthreads();
  }
  if (live) {
    if (MODE == CSR_RESID || MODE == CSR_SPMV) {
      out[row] = acc;
    } else if (MODE == CSR_SPMV_ADD) {
      out[row] = fi + acc;  // t = P u_H summed from 0, then u_h + t: the reference's two statements
    } else if (MODE == CSR_JACOBI) {
      out[row] = (diag == 0.0) ? xi : xi + omega * ((fi - acc) / diag - xi);
    } else if (mode_cheb(MODE)) {
      double dn;
      out[row] = cheb_update<MODE>((diag == 0.0) ? xi : (fi - acc) / diag, xi, di, alpha, omega, dn);
      if (!cheb_last(MODE)) dvec[row] = dn;
    } else {  // CSR_RSSQ: (b - bhat)^2, common.hpp:24
      const double d = fi - acc;
      out[row] = d * d;
    }
  }
}

template <int MODE, int K, int U>
static hipError_t launch_csr_ku(int64_t n, int64_t nnz, const int32_t* rowptr,
                                const int32_t* col, const double* val,
                                const double* x, const double* f, double* out,
                                double omega, int64_t diag_shift, hipStream_t st,
                                double* dvec = nullptr, double alpha = 0.0) {
  if (n <= 0) return hipSuccess;
  const size_t lds = (size_t)(CSR_BLOCK * K + 4) * 12;
  const unsigned grid = (unsigned)((n + CSR_BLOCK - 1) / CSR_BLOCK);
  hipLaunchKernelGGL((csr_stage_kernel<MODE, K, U>), dim3(grid), dim3(CSR_BLOCK), lds,
                     st, n, nnz, rowptr, col, val, x, f, out, omega, diag_shift, dvec, alpha);
  return hipGetLastError();
}

template <int MODE>
static hipError_t launch_csr_mode(int64_t n, int64_t nnz, int max_block_nnz,
                                  int max_row_nnz, const int32_t* rowptr,
                                  const int32_t* col, const double* val,
                                  const double* x, const double* f, double* out,
                                  double omega, int64_t diag_shift, hipStream_t st,
                                  double* dvec = nullptr, double alpha = 0.0) {
  // +3: the chunk start is rounded down to a multiple of 4 entries.  U (gathers
  // issued per pass of a lane over its row) is matched to the longest row: a
  // 5-point row walked with U = 8 wastes 3 LDS reads + 3 gathers (measured
  // 4.9 -> 5.6 TB/s on the 4096^2 fine level, tools/kbench.hip).
  const int need = max_block_nnz + 3;
  if (need <= CSR_BLOCK * 4 && max_row_nnz <= 3)
    return launch_csr_ku<MODE, 4, 3>(n, nnz, rowptr, col, val, x, f, out, omega, diag_shift, st, dvec,
                                      alpha);
  if (need <= CSR_BLOCK * 6 && max_row_nnz <= 5)
    return launch_csr_ku<MODE, 6, 5>(n, nnz, rowptr, col, val, x, f, out, omega, diag_shift, st, dvec,
                                      alpha);
  if (need <= CSR_BLOCK * 8 && max_row_nnz <= 7)
    return launch_csr_ku<MODE, 8, 7>(n, nnz, rowptr, col, val, x, f, out, omega, diag_shift, st, dvec,
                                      alpha);
  if (need <= CSR_BLOCK * 10 && max_row_nnz <= 9)
    return launch_csr_ku<MODE, 10, 9>(n, nnz, rowptr, col, val, x, f, out, omega, diag_shift, st, dvec,
                                      alpha);
  return launch_csr_ku<MODE, 16, 8>(n, nnz, rowptr, col, val, x, f, out, omega, diag_shift, st, dvec,
                                      alpha);
}

hipError_t launch_csr(int mode, int64_t n, int64_t nnz, int max_block_nnz,
                      int max_row_nnz, const int32_t* rowptr, const int32_t* col,
                      const double* val, const double* x, const double* f,
                      double* out, double omega, int64_t diag_shift, hipStream_t st) {
  switch (mode) {
    case CSR_RESID:
      return launch_csr_mode<CSR_RESID>(n, nnz, max_block_nnz, max_row_nnz, rowptr, col,
                                        val, x, f, out, omega, diag_shift, st);
    case CSR_JACOBI:
      return launch_csr_mode<CSR_JACOBI>(n, nnz, max_block_nnz, max_row_nnz, rowptr, col,
                                         val, x, f, out, omega, diag_shift, st);
    case CSR_SPMV:
      return launch_csr_mode<CSR_SPMV>(n, nnz, max_block_nnz, max_row_nnz, rowptr, col,
                                       val, x, f, out, omega, diag_shift, st);
    case CSR_RSSQ:
      return launch_csr_mode<CSR_RSSQ>(n, nnz, max_block_nnz, max_row_nnz, rowptr, col,
                                       val, x, f, out, omega, diag_shift, st);
    case CSR_SPMV_ADD:
      return launch_csr_mode<CSR_SPMV_ADD>(n, nnz, max_block_nnz, max_row_nnz, rowptr, col,
                                           val, x, f, out, omega, diag_shift, st);
  }
  return hipErrorInvalidValue;
}
hipError_t launch_csr_cheb(int64_t n, int64_t nnz, int max_block_nnz, int max_row_nnz, const int32_t* rowptr,
                           const int32_t* col, const double* val, const double* x, const double* f, double* out,
                           const ChebStep& c, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (!c.d || x == out) return hipErrorInvalidValue;
#define AMG_CSR_CHEB(FI, LA)                                                                            \
  return launch_csr_mode<cheb_kernel_mode(FI, LA)>(n, nnz, max_block_nnz, max_row_nnz, rowptr, col, val, x, f, \
                                                   out, c.beta, 0, st, c.d, c.alpha)
  if (c.first && c.last) AMG_CSR_CHEB(true, true);
  if (c.first) AMG_CSR_CHEB(true, false);
  if (c.last) AMG_CSR_CHEB(false, true);
  AMG_CSR_CHEB(false, false);
#undef AMG_CSR_CHEB
}

// Gershgorin bound (kernels.hpp: launch_gershgorin): one lane per row, ascending column order as
// the host sums; the max is order-independent, so the bound has the host's bits.  Non-negative
// doubles order like their bit patterns: the block maximum goes out as one 64-bit atomic max.
__global__ __launch_bounds__(256) void gershgorin_kernel(int64_t n, const int32_t* __restrict__ rowptr,
                                                         const int32_t* __restrict__ col,
                                                         const double* __restrict__ val,
                                                         unsigned long long* out) {
  __shared__ double red[256];
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  double g = 0.0;
  if (row < n) {
    double sum = 0.0, dg = 0.0;
    for (int32_t p = rowptr[row]; p < rowptr[row + 1]; ++p) {
      const double v = val[p];
      sum += fabs(v);
      if ((int64_t)col[p] == row) dg = v;
    }
    if (dg == 0.0) atomicMin(out + 1, (unsigned long long)row);
    else g = sum / fabs(dg);
    if (!(g >= 0.0)) g = 0.0;  // NaN rows do not bound anything
  }
  red[threadIdx.x] = g;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + w]);
    __syncthreads();
  }
  if (threadIdx.x == 0) atomicMax(out, (unsigned long long)__double_as_longlong(red[0]));
}
__global__ void gershgorin_init_kernel(unsigned long long* out) {
  if (threadIdx.x < 2) out[threadIdx.x] = threadIdx.x == 0 ? 0ull : ~0ull;
}
hipError_t launch_gershgorin(int64_t n, const int32_t* rowptr, const int32_t* col, const double* val,
                             uint64_t* out, hipStream_t st) {
  hipLaunchKernelGGL(gershgorin_init_kernel, dim3(1), dim3(64), 0, st, reinterpret_cast<unsigned long long*>(out));
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || n <= 0) return e;
  hipLaunchKernelGGL(gershgorin_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, rowptr, col, val,
                     reinterpret_cast<unsigned long long*>(out));
  return hipGetLastError();
}

// K-AxisStrength (kernels.hpp: launch_axis_strength): per grid axis the maximum of |a_ij| over the
// entries whose column is the row's neighbour along that axis alone; one lane per row.  Like the
// Gershgorin bound: a maximum of non-negative doubles is order-independent and orders like the bit
// patterns, so the three block maxima go out as 64-bit atomic maxima and equal the host's bits.
__global__ __launch_bounds__(256) void axis_strength_kernel(uint32_t n, uint32_t nx, uint32_t ny,
                                                            const int32_t* __restrict__ rowptr,
                                                            const int32_t* __restrict__ col,
                                                            const double* __restrict__ val,
                                                            unsigned long long* out) {
  __shared__ double red[3][256];
  const uint32_t row = blockIdx.x * 256u + threadIdx.x;
  double w[3] = {0.0, 0.0, 0.0};
  if (row < n) {
    const uint32_t ri = row % nx, rq = row / nx, rj = rq % ny, rk = rq / ny;
    for (int32_t p = rowptr[row], e = rowptr[row + 1]; p < e; ++p) {
      const uint32_t c = (uint32_t)col[p];
      const uint32_t ci = c % nx, cq = c / nx, cj = cq % ny, ck = cq / ny;
      const int32_t dx = (int32_t)ci - (int32_t)ri, dy = (int32_t)cj - (int32_t)rj, dz = (int32_t)ck - (int32_t)rk;
      const int32_t ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy, az = dz < 0 ? -dz : dz;
      if (ax + ay + az != 1) continue;
      const double v = fabs(val[p]);
      if (ax) { if (v > w[0]) w[0] = v; }
      else if (ay) { if (v > w[1]) w[1] = v; }
      else { if (v > w[2]) w[2] = v; }
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) red[a][threadIdx.x] = w[a];
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) {
#pragma unroll
      for (int a = 0; a < 3; ++a) red[a][threadIdx.x] = fmax(red[a][threadIdx.x], red[a][threadIdx.x + h]);
    }
    __syncthreads();
  }
  if (threadIdx.x < 3) atomicMax(out + threadIdx.x, (unsigned long long)__double_as_longlong(red[threadIdx.x][0]));
}
__global__ void axis_strength_init_kernel(unsigned long long* out) {
  if (threadIdx.x < 3) out[threadIdx.x] = 0ull;
}
hipError_t launch_axis_strength(int64_t n, int dim, const int64_t dims[3], const int32_t* rowptr, const int32_t* col,
                                const double* val, uint64_t* out, hipStream_t st) {
  if ((dim != 2 && dim != 3) || !dims || dims[0] < 1 || dims[1] < 1 || dims[2] < 1 ||
      n != dims[0] * dims[1] * dims[2] || n >= ((int64_t)1 << 31))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(axis_strength_init_kernel, dim3(1), dim3(64), 0, st, reinterpret_cast<unsigned long long*>(out));
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(axis_strength_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (uint32_t)n,
                     (uint32_t)dims[0], (uint32_t)dims[1], rowptr, col, val, reinterpret_cast<unsigned long long*>(out));
  return hipGetLastError();
}

// ---------------------------------------------------------------- K-SELL -----
// Same four operations on the solver's own level matrices, stored as CSR sliced
// into 64-row panels with each panel lane-interleaved (SELL-64): entry j of row
// r sits at soff[r/64] + 64*j + (r%64), rows padded to the panel's longest row
// with col = -1.  One lane per row; every load of a wave is one contiguous
// 256-B (col) / 512-B (val) segment, no row pointer, no LDS round trip, no
// barrier, ascending-column order per row kept (bit-identical results to K-CSR).
// Measured on the 4096^2 fine level: 6.2 TB/s algorithmic vs 5.6 TB/s for K-CSR
// (tools/kbench.hip) -- the panel layout is what "CSR laid out for coalesced
// HBM reads" comes to on wave64 hardware.
// MODE CSR_GS (multicolour Gauss-Seidel): rows are the colour-permuted rows
// [row0, row0 + count) of the matrix, rowid[p] is the dof each one updates
// (-1 = padding), x is updated IN PLACE -- rows of one colour do not reference
// each other, so the launch is race-free.
// IDX16: column indices stored as 16-bit offsets from the row's diagonal column
// (col - (row + dshift)), pad = -32768.  Every level of a banded hierarchy with
// half-bandwidth < 32768 qualifies; 10 instead of 12 bytes per entry, and a wave's
// index load is exactly one 128-B line.
// NT: the matrix stream (index, value), f and the output use non-temporal
// accesses, so that the once-read stream does not evict the x lines the gathers
// re-use from L2 (measured 229 -> 208 us on the 4096^2 fine level).  Only for
// matrices far larger than the Infinity Cache; small levels keep the default
// policy because their matrix is re-read from cache by the next sweep.
template <int MODE, bool IDX16, bool NT>
__global__ __launch_bounds__(256) void sell_kernel(
    int n, const int64_t* __restrict__ soff, const void* __restrict__ scol_v,
    const double* __restrict__ sval, const double* x, const double* __restrict__ f,
    double* out, double omega, const int32_t* __restrict__ rowid, int row0,
    const double* __restrict__ uH, int nH, int dshift, double* dvec, double alpha) {
  // CSR_JACOBI_P: x is not the smoother's input yet -- the input is x + P uH
  // (LinearInterpolator prolongation, interpolator.hpp:106-129), formed on the
  // fly per gathered entry in the same order as K-ProlongAdd:
  //   t[2j+1] = 0 + 1.0 uH[j];  t[2j] = (0 + 0.5 uH[j-1]) + 0.5 uH[j].
  auto corrected = [&](int c) -> double {
    const double xc = x[c];
    const int j = c >> 1;
    const double a = uH[(j >= 1 && j - 1 < nH) ? j - 1 : 0];
    const double b = uH[j < nH ? j : 0];
    double t = 0.0;
    if (c & 1) {
      if (j < nH) t += 1.0 * b;
    } else {
      if (j >= 1 && j - 1 < nH) t += 0.5 * a;
      if (j < nH) t += 0.5 * b;
    }
    return xc + t;
  };
  const int32_t* __restrict__ scol = static_cast<const int32_t*>(scol_v);
  const int16_t* __restrict__ scol16 = static_cast<const int16_t*>(scol_v);
  const int p = row0 + blockIdx.x * 256 + threadIdx.x;  // storage row
  const int s = p >> 6;
  if ((s << 6) >= n) return;  // whole wave past the end
  const int64_t o0 = soff[s], o1 = soff[s + 1];
  const int w = (int)((o1 - o0) >> 6);  // wave-uniform panel width
  const int64_t base = o0 + (p & 63);
  int row = p;
  bool live = p < n;
  if (MODE == CSR_GS) {
    row = live ? rowid[p] : -1;
    live = row >= 0;
  }
  // column of row's diagonal: row itself, or row + dshift when x is a rank's
  // halo-extended vector and the columns are numbered in it (multi-GPU shards)
  const int drow = row + dshift;
  double fi = 0.0, xi = 0.0, di = 0.0;
  if (live) {
    if (MODE != CSR_SPMV) fi = NT ? __builtin_nontemporal_load(f + row) : f[row];
    if (mode_jac(MODE) || MODE == CSR_GS) xi = x[drow];
    if (MODE == CSR_JACOBI_P) xi = corrected(row);
    if (mode_cheb(MODE) && !cheb_first(MODE)) di = NT ? __builtin_nontemporal_load(dvec + row) : dvec[row];
  }
  double acc = (MODE == CSR_RESID) ? fi : 0.0;
  double diag = 0.0;
  // one pass over U entries: all loads of the pass are issued before the first use
  auto pass = [&](int j0, auto UU) {
    constexpr int UN = decltype(UU)::value;
    int32_t c[UN];
    double v[UN], xx[UN];
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int j = j0 + u < w ? j0 + u : j0;
      const int64_t at = base + ((int64_t)j << 6);
      if (IDX16) {
        const int d = NT ? __builtin_nontemporal_load(scol16 + at) : scol16[at];
        c[u] = (d == -32768) ? -1 : drow + d;
      } else {
        c[u] = NT ? __builtin_nontemporal_load(scol + at) : scol[at];
      }
      v[u] = NT ? __builtin_nontemporal_load(sval + at) : sval[at];
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      if (MODE == CSR_JACOBI_P) xx[u] = corrected(c[u] >= 0 ? c[u] : 0);
      else xx[u] = x[c[u] >= 0 ? c[u] : 0];
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      if (j0 + u < w && c[u] >= 0) {
        if (MODE == CSR_RESID) {
          acc -= v[u] * xx[u];
        } else if (mode_jac(MODE) || MODE == CSR_GS || MODE == CSR_JACOBI_P) {
          if (c[u] == drow) diag = v[u];
          else acc += v[u] * xx[u];
        } else {
          acc += v[u] * xx[u];
        }
      }
    }
  };
  // the pass length follows the PANEL's width (wave-uniform branch): a 7-wide
  // panel walked with a 9-entry pass would issue 2 dead loads + 2 dead gathers.
  // A panel of empty rows (w == 0) owns no slot: soff[s] is the next panel's first slot, or
  // `slots` itself for a trailing one, so no pass may run (a pass clamps j to j0 and loads)
  if (w == 0) {
  } else if (w <= 3) pass(0, std::integral_constant<int, 3>{});
  else if (w <= 5) pass(0, std::integral_constant<int, 5>{});
  else if (w <= 7) pass(0, std::integral_constant<int, 7>{});
  else if (w <= 9) pass(0, std::integral_constant<int, 9>{});
  else
    for (int j0 = 0; j0 < w; j0 += 8) pass(j0, std::integral_constant<int, 8>{});
  if (live) {
    double res;
    bool store = true;
    if (MODE == CSR_RESID || MODE == CSR_SPMV) {
      res = acc;
    } else if (MODE == CSR_JACOBI || MODE == CSR_JACOBI_P) {
      res = (diag == 0.0) ? xi : xi + omega * ((fi - acc) / diag - xi);
    } else if (mode_cheb(MODE)) {
      double dn;
      res = cheb_update<MODE>((diag == 0.0) ? xi : (fi - acc) / diag, xi, di, alpha, omega, dn);
      if (!cheb_last(MODE)) {
        if (NT) __builtin_nontemporal_store(dn, dvec + row);
        else dvec[row] = dn;
      }
    } else if (MODE == CSR_GS) {
      res = (fi - acc) / diag;  // smoother.hpp:136
      store = diag != 0.0;
    } else {
      const double d = fi - acc;
      res = d * d;
    }
    if (store) {
      if (NT && MODE != CSR_GS) __builtin_nontemporal_store(res, out + row);
      else out[row] = res;
    }
  }
}

template <int MODE>
static hipError_t launch_sell_mode(int64_t n, int idx16, const int64_t* soff,
                                   const void* scol, const double* sval, const double* x,
                                   const double* f, double* out, double omega,
                                   const int32_t* rowid, int64_t row0, int64_t count,
                                   const double* uH, int64_t nH, hipStream_t st,
                                   int64_t diag_shift = 0, double* dvec = nullptr, double alpha = 0.0) {
  const unsigned grid = (unsigned)((count + 255) / 256);
  // idx16: bit 0 = 16-bit relative columns, bit 1 = non-temporal matrix stream
#define AMG_SELL_LAUNCH(I16, NTF)                                                              \
  hipLaunchKernelGGL((sell_kernel<MODE, I16, NTF>), dim3(grid), dim3(256), 0, st, (int)n, soff, \
                     scol, sval, x, f, out, omega, rowid, (int)row0, uH, (int)nH, (int)diag_shift, dvec, alpha)
  switch (idx16 & 3) {
    case 0: AMG_SELL_LAUNCH(false, false); break;
    case 1: AMG_SELL_LAUNCH(true, false); break;
    case 2: AMG_SELL_LAUNCH(false, true); break;
    default: AMG_SELL_LAUNCH(true, true); break;
  }
#undef AMG_SELL_LAUNCH
  return hipGetLastError();
}
hipError_t launch_sell(int mode, int64_t n, int idx16, const int64_t* soff,
                       const void* scol, const double* sval, const double* x,
                       const double* f, double* out, double omega, int64_t diag_shift,
                       hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (n >= ((int64_t)1 << 31) - 256 || diag_shift >= ((int64_t)1 << 30)) return hipErrorInvalidValue;
  switch (mode) {
    case CSR_RESID: return launch_sell_mode<CSR_RESID>(n, idx16, soff, scol, sval, x, f, out, omega, nullptr, 0, n, nullptr, 0, st, diag_shift);
    case CSR_JACOBI: return launch_sell_mode<CSR_JACOBI>(n, idx16, soff, scol, sval, x, f, out, omega, nullptr, 0, n, nullptr, 0, st, diag_shift);
    case CSR_SPMV: return launch_sell_mode<CSR_SPMV>(n, idx16, soff, scol, sval, x, f, out, omega, nullptr, 0, n, nullptr, 0, st, diag_shift);
    case CSR_RSSQ: return launch_sell_mode<CSR_RSSQ>(n, idx16, soff, scol, sval, x, f, out, omega, nullptr, 0, n, nullptr, 0, st, diag_shift);
  }
  return hipErrorInvalidValue;
}

hipError_t launch_sell_cheb(int64_t n, int idx16, const int64_t* soff, const void* scol, const double* sval,
                            const double* x, const double* f, double* out, const ChebStep& c, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (n >= ((int64_t)1 << 31) - 256 || !c.d || x == out) return hipErrorInvalidValue;
#define AMG_SELL_CHEB(FI, LA)                                                                                \
  return launch_sell_mode<cheb_kernel_mode(FI, LA)>(n, idx16, soff, scol, sval, x, f, out, c.beta, nullptr, 0, n, \
                                                    nullptr, 0, st, 0, c.d, c.alpha)
  if (c.first && c.last) AMG_SELL_CHEB(true, true);
  if (c.first) AMG_SELL_CHEB(true, false);
  if (c.last) AMG_SELL_CHEB(false, true);
  AMG_SELL_CHEB(false, false);
#undef AMG_SELL_CHEB
}

hipError_t launch_sell_jacobi_prolong(int64_t n, int idx16, const int64_t* soff,
                                      const void* scol, const double* sval, const double* u,
                                      const double* uH, int64_t nH, const double* f, double* out,
                                      double omega, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (n >= ((int64_t)1 << 31) - 256 || nH < 1) return hipErrorInvalidValue;
  return launch_sell_mode<CSR_JACOBI_P>(n, idx16, soff, scol, sval, u, f, out, omega, nullptr,
                                        0, n, uH, nH, st);
}

hipError_t launch_sell_gs_color(int64_t n_storage, int /*idx16: rows are permuted*/,
                                const int64_t* soff, const int32_t* scol, const double* sval,
                                const int32_t* rowid,
                                int64_t row0, int64_t count, const double* f, double* u,
                                hipStream_t st) {
  if (count <= 0) return hipSuccess;
  if (n_storage >= ((int64_t)1 << 31) - 256 || (row0 & 63)) return hipErrorInvalidValue;
  // the kernel's row bound is the END OF THIS COLOUR: a 256-thread workgroup must not run on
  // into the storage rows of the next colour (they reference this colour's rows)
  const int64_t end = row0 + count < n_storage ? row0 + count : n_storage;
  return launch_sell_mode<CSR_GS>(end, 0, soff, scol, sval, u, f, u, 1.0, rowid, row0,
                                  count, nullptr, 0, st);
}

static int g_dict_rows_per_lane = 2;
static int g_xcd_map = 1;
// ---------------------------------------------------------------- K-Dict -----
// The same four operations on a dictionary-coded matrix (host_setup.hpp: DictMat).
// Lane per row; the row's structure is ONE 8- or 16-byte load (byte j = code of
// entry j, 0xFF = none), the <= 255 (column offset, value) pairs live in LDS.  The
// matrix stream shrinks from 10-12 bytes per entry to 8/16 bytes per row, which on
// the 4096^2 fine level leaves f, x and the output as the bulk of the HBM traffic.
// Entry order (ascending column) and the decoded doubles are the stored ones, so
// results are bit-identical to K-SELL / K-CSR.
// R = rows per lane (1 or 2).  R = 2: a lane owns rows 2t and 2t+1, so codes, f and
// the output move as 16-byte (32-byte for two-word codes) lane accesses and twice as
// many bytes are in flight per wave (the launcher checks the 16-byte alignment).
// (Persistent workgroups that prefetch their next tile were measured 10 % SLOWER on the
// 4096^2 fine level, 108 vs 99 us, and are not kept.)
// Row types (second-level dictionary): the rows of such a matrix also repeat as whole
// code words (2-D Poisson hierarchy: <= 12 distinct rows per level, 3-D: <= 40), so
// when there are at most 255 distinct words a row is ONE byte indexing a word table in
// LDS (type 255 = empty row), and the matrix stream is 1 byte per row.
template <int WORDS, int R>
struct DictStream {  // streamed operands of R rows of one lane
  uint64_t cw[R][2];
  uint32_t ty;  // row types, byte r = row r
  double fi[R], xi[R];
  double di[R];  // Chebyshev steps after the first: d_i
  bool live[R];
};
template <int MODE, int WORDS, bool NT, int R>
__device__ __forceinline__ void dict_fetch(DictStream<WORDS, R>& s, int row0, int n,
                                           const uint64_t* __restrict__ codes,
                                           const uint8_t* __restrict__ rtype,
                                           const double* __restrict__ f, const double* x,
                                           int dshift, const double* __restrict__ dvec = nullptr) {
  typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));
  typedef double f64x2 __attribute__((ext_vector_type(2)));
  constexpr bool read_d = mode_cheb(MODE) && !cheb_first(MODE);
#pragma unroll
  for (int r = 0; r < R; ++r) {
    s.live[r] = row0 + r < n;
    s.cw[r][0] = s.cw[r][1] = ~(uint64_t)0;
    s.fi[r] = s.xi[r] = s.di[r] = 0.0;
  }
  s.ty = 0xFFFFu;  // both rows empty; unpacked in dict_expand, after the other loads are out
  if (R == 2 && s.live[R - 1]) {
    if (rtype) {  // wave-uniform
      s.ty = *reinterpret_cast<const uint16_t*>(rtype + row0);
    } else {
      const u64x2* vp = reinterpret_cast<const u64x2*>(codes + (int64_t)row0 * WORDS);
      const u64x2 a = NT ? __builtin_nontemporal_load(vp) : *vp;
      if (WORDS == 2) {
        const u64x2 b2 = NT ? __builtin_nontemporal_load(vp + 1) : vp[1];
        s.cw[0][0] = a.x; s.cw[0][1] = a.y; s.cw[R - 1][0] = b2.x; s.cw[R - 1][1] = b2.y;
      } else {
        s.cw[0][0] = a.x; s.cw[R - 1][0] = a.y;
      }
    }
    if (MODE != CSR_SPMV) {
      const f64x2* fp = reinterpret_cast<const f64x2*>(f + row0);
      const f64x2 t = NT ? __builtin_nontemporal_load(fp) : *fp;
      s.fi[0] = t.x; s.fi[R - 1] = t.y;
    }
    if (mode_jac(MODE)) { s.xi[0] = x[row0 + dshift]; s.xi[R - 1] = x[row0 + 1 + dshift]; }
    if (read_d) {
      const f64x2* dp = reinterpret_cast<const f64x2*>(dvec + row0);
      const f64x2 t = NT ? __builtin_nontemporal_load(dp) : *dp;
      s.di[0] = t.x; s.di[R - 1] = t.y;
    }
  } else if (s.live[0]) {
    if (rtype) {
      s.ty = 0xFF00u | rtype[row0];
    } else {
      const uint64_t* cp = codes + (int64_t)row0 * WORDS;
      if (WORDS == 2) {
        const u64x2* vp = reinterpret_cast<const u64x2*>(cp);
        const u64x2 t = NT ? __builtin_nontemporal_load(vp) : *vp;
        s.cw[0][0] = t.x; s.cw[0][1] = t.y;
      } else {
        s.cw[0][0] = NT ? __builtin_nontemporal_load(cp) : cp[0];
      }
    }
    if (MODE != CSR_SPMV) s.fi[0] = NT ? __builtin_nontemporal_load(f + row0) : f[row0];
    if (mode_jac(MODE)) s.xi[0] = x[row0 + dshift];
    if (read_d) s.di[0] = NT ? __builtin_nontemporal_load(dvec + row0) : dvec[row0];
  }
}
// word table of the row types: 256 entries of WORDS words, entry 255 = all 0xFF (host pads)
template <int WORDS>
__device__ __forceinline__ void dict_stage_words(uint64_t* wtab, const uint64_t* __restrict__ rwords) {
#pragma unroll
  for (int k = 0; k < WORDS; ++k) wtab[threadIdx.x * WORDS + k] = rwords[threadIdx.x * WORDS + k];
}
template <int WORDS, int R>
__device__ __forceinline__ void dict_expand(DictStream<WORDS, R>& s, const uint64_t* wtab) {
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int k = 0; k < WORDS; ++k) s.cw[r][k] = wtab[((s.ty >> (8 * r)) & 0xFFu) * WORDS + k];
}
// One 32-byte LDS entry per code.  Entry 255 (= no entry) is all zero: its gather reads
// the row's diagonal column (always a valid address).
// Jacobi sweeps stage  a = value of an OFF-diagonal pair (else +0.0),
//                      d = value of a diagonal pair (else +0.0);
// the other modes      a = value.
struct DictEntry {
  double a;
  double d;
  int32_t off8;  // BYTE offset of the column from the row's diagonal column
  int32_t pad[3];
};
// entry threadIdx.x from its pair (v, o), already in registers
template <int MODE>
__device__ __forceinline__ void dict_put_table(DictEntry* tab, double v, int32_t o, int ntab) {
  const int t = threadIdx.x;  // 256 threads, 256 entries
  DictEntry e;
  constexpr bool split = mode_jac(MODE) || MODE == CSR_GS;
  e.a = (split && o == 0) ? 0.0 : v;
  e.d = (split && o == 0 && t < ntab) ? v : 0.0;
  e.off8 = o * 8;
  e.pad[0] = e.pad[1] = e.pad[2] = 0;
  tab[t] = e;
}
template <int MODE>
__device__ __forceinline__ void dict_stage_table(DictEntry* tab, const int32_t* __restrict__ doff,
                                                 const double* __restrict__ dval, int ntab) {
  const int t = threadIdx.x;
  const double v = t < ntab ? dval[t] : 0.0;
  const int32_t o = t < ntab ? doff[t] : 0;
  dict_put_table<MODE>(tab, v, o, ntab);
}
// decode + gather + row arithmetic of the R rows of one lane.  The kernels are issue
// bound as much as bandwidth bound (a wave64 VALU instruction occupies its SIMD for 4
// cycles), so the row walk is branch-free and short: per entry one byte extract, one
// 16-byte + one 4-byte LDS read, one 32-bit add for the byte offset (the gather uses
// the scalar-base + 32-bit-offset addressing mode), mul, add.
//
// Skipped terms and bit-identity.  A Jacobi sweep adds (+0.0) * x for "no entry" slots
// and for the diagonal pair, i.e. +-0.0 for finite x: acc + (+-0.0) == acc because a sum
// that starts at +0.0 is never -0.0, and diag + (+0.0) == diag, so for finite vectors
// the result has the same bits as skipping those terms (the x read there is the row's
// own u_i, which enters the result anyway).  The other modes skip "no entry" slots
// with a select: acc - (+0.0) == acc holds for every acc.
template <int MODE, int WORDS, int UN, int R>
__device__ __forceinline__ void dict_rows(const DictStream<WORDS, R>& s, int row0,
                                          const DictEntry* tab, const double* x, double omega,
                                          int dshift, double (&res)[R]) {
  uint32_t c8[R][UN];
  double v[R][UN], vd[R][UN], xx[R][UN];
  bool ok[R][UN];
  const char* xb = reinterpret_cast<const char*>(x);
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const uint32_t drow8 = s.live[r] ? (uint32_t)(row0 + r + dshift) * 8u : 0u;
    const uint32_t w32[4] = {(uint32_t)s.cw[r][0], (uint32_t)(s.cw[r][0] >> 32),
                             (uint32_t)s.cw[r][1], (uint32_t)(s.cw[r][1] >> 32)};
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const uint32_t code = (w32[u >> 2] >> (8 * (u & 3))) & 0xFFu;
      ok[r][u] = code != 0xFFu;
      c8[r][u] = drow8 + (uint32_t)tab[code].off8;
      v[r][u] = tab[code].a;
      vd[r][u] = (mode_jac(MODE) || MODE == CSR_GS) ? tab[code].d : 0.0;
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int u = 0; u < UN; ++u)
      xx[r][u] = *reinterpret_cast<const double*>(xb + c8[r][u]);
#pragma unroll
  for (int r = 0; r < R; ++r) {
    double acc = (MODE == CSR_RESID) ? s.fi[r] : 0.0;
    double diag = 0.0;
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      double t = v[r][u] * xx[r][u];
      if (mode_jac(MODE) || MODE == CSR_GS) {
        acc += t;
        diag += vd[r][u];
      } else {
        // the empty asm keeps the product unconditional, so that clang does not turn
        // the select into an exec-masked branch with the gather (and its wait) inside
        asm volatile("" : "+v"(t));
        t = ok[r][u] ? t : 0.0;
        if (MODE == CSR_RESID) acc -= t;
        else acc += t;
      }
    }
    if (MODE == CSR_RESID || MODE == CSR_SPMV) {
      res[r] = acc;
    } else if (mode_jac(MODE) || MODE == CSR_GS) {
      // The division runs for every row (a missing diagonal divides by 1 and is then
      // discarded): with it inside `diag != 0` clang puts the whole row walk, gathers and
      // their waits included, into that branch and the rows of a lane run one after
      // the other instead of overlapping.
      const bool nod = diag == 0.0;
      double q = (s.fi[r] - acc) / (nod ? 1.0 : diag);  // smoother.hpp:136
      asm volatile("" : "+v"(q));
      if (MODE == CSR_GS || mode_cheb(MODE)) res[r] = nod ? s.xi[r] : q;  // Chebyshev: t_i (cheb_update)
      else res[r] = nod ? s.xi[r] : s.xi[r] + omega * (q - s.xi[r]);
    } else {
      const double d = s.fi[r] - acc;
      res[r] = d * d;
    }
  }
}
// Wave-uniform STENCIL rows (the interior of a 3-D level: almost every wave).  When all 128 rows of
// a wave share one row type whose columns are the 7-point pattern {-M, -m, -1, 0, +1, +m, +M} or the
// 15-point pattern {-M, -m, 0, +m, +M} x {-1, 0, +1} (m, M even), a lane's two consecutive rows need
// 12 / 20 distinct entries of x that sit in aligned pairs: 7 / 15 load instructions (16-byte pairs
// plus the two outer singles of a triple) instead of the 16 / 32 eight-byte gathers of dict_rows --
// the sweeps of these levels are bound by the gathers through the vector L1, not by HBM (traffic
// 1.01 x must-move at 3.9 / 2.4 TB/s) and not by the decode (a scalar-table path with the same
// gathers measured no faster).  Values come through scalar loads from a per-type table (utd: per
// type {off-diagonal value or +0.0 [16], value [16], diagonal}, uti: {offset in rows [16], mask of
// slots in use, pattern 7 / 15 / 0}), built by the host from the same pairs.  Same products in the
// same slot order: Jacobi adds (+0.0) x for the diagonal slot exactly as dict_rows does -> same
// bits.  A mixed wave, or one whose type has no pattern, takes dict_rows (dict_stencil_can).
// (wave-uniform) does this wave qualify?  (Deciding this per WORKGROUP before the LDS tables are
// staged, so that a workgroup of stencil waves skips the staging -- 12 KB of loads and LDS stores
// per 512 rows --, was measured no faster: 512^3 +3.2 % against +5.2 % for this form; the early
// workgroup-wide vote waits for the row types with nothing else in flight.)
template <int UN>
__device__ __forceinline__ bool dict_stencil_can(uint32_t ty, const bool (&live)[2],
                                                 const int32_t* __restrict__ uti) {
  constexpr int PAT = UN == 7 ? 7 : 15;
  const uint32_t t0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(ty & 0xFFu));
  const bool ok = ty == (t0 | (t0 << 8)) && live[0] && live[1];
  if (t0 == 255u || __builtin_amdgcn_ballot_w64(!ok) != 0) return false;
  return uti[t0 * 18u + 17u] == PAT;
}
template <int MODE, int UN>
__device__ __forceinline__ void dict_rows_stencil(uint32_t ty, const double (&fi)[2],
                                                  const double (&xi)[2], int row0,
                                                  const double* __restrict__ utd,
                                                  const int32_t* __restrict__ uti, const double* x,
                                                  double omega, double (&res)[2]) {
  static_assert(mode_jac(MODE) || MODE == CSR_RESID, "fast path of the hot modes");
  static_assert(UN == 7 || UN == 16, "7-point rows / 15-point rows");
  typedef double f64x2 __attribute__((ext_vector_type(2)));
  constexpr int PAT = UN == 7 ? 7 : 15;
  const uint32_t t0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(ty & 0xFFu));
  const int32_t* ti = uti + t0 * 18u;
  const double* td = utd + t0 * 33u + (MODE == CSR_RESID ? 16u : 0u);
  const double* xr = x + row0;  // row0 is even, x 16-byte aligned, m and M even
  double xx[2][PAT];
  if (PAT == 7) {
    const int g[4] = {0, 1, 5, 6};  // slots of -M, -m, +m, +M
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const f64x2 v = *reinterpret_cast<const f64x2*>(xr + ti[g[k]]);
      xx[0][g[k]] = v.x;
      xx[1][g[k]] = v.y;
    }
    const f64x2 c = *reinterpret_cast<const f64x2*>(xr);
    const double lo = xr[-1], hi = xr[2];
    xx[0][2] = lo;  xx[0][3] = c.x; xx[0][4] = c.y;
    xx[1][2] = c.x; xx[1][3] = c.y; xx[1][4] = hi;
  } else {
#pragma unroll
    for (int k = 0; k < 5; ++k) {  // triple k: slots 3k, 3k+1, 3k+2 around the offset of slot 3k+1
      const double* xc = xr + ti[3 * k + 1];
      const f64x2 c = *reinterpret_cast<const f64x2*>(xc);
      const double lo = xc[-1], hi = xc[2];
      xx[0][3 * k] = lo;  xx[0][3 * k + 1] = c.x; xx[0][3 * k + 2] = c.y;
      xx[1][3 * k] = c.x; xx[1][3 * k + 1] = c.y; xx[1][3 * k + 2] = hi;
    }
  }
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    double acc = (MODE == CSR_RESID) ? fi[r] : 0.0;
#pragma unroll
    for (int u = 0; u < PAT; ++u) {
      const double t = td[u] * xx[r][u];
      if (mode_jac(MODE)) acc += t;       // td[u] = +0.0 for the diagonal slot (dict_stage_table<CSR_JACOBI>)
      else acc -= t;                      // every slot of the pattern is in use
    }
    if (MODE == CSR_RESID) {
      res[r] = acc;
    } else {
      const double diag = td[32];
      const bool nod = diag == 0.0;
      const double q = (fi[r] - acc) / (nod ? 1.0 : diag);  // smoother.hpp:136
      if (mode_cheb(MODE)) res[r] = nod ? xi[r] : q;  // t_i (cheb_update)
      else res[r] = nod ? xi[r] : xi[r] + omega * (q - xi[r]);
    }
  }
}
template <int WORDS, bool NT, int R>
__device__ __forceinline__ void dict_store(const DictStream<WORDS, R>& s, int row0,
                                           const double (&res)[R], double* out) {
  typedef double f64x2 __attribute__((ext_vector_type(2)));
  if (R == 2 && s.live[R - 1]) {
    f64x2 t;
    t.x = res[0]; t.y = res[R - 1];
    f64x2* op = reinterpret_cast<f64x2*>(out + row0);
    if (NT) __builtin_nontemporal_store(t, op);
    else *op = t;
  } else if (s.live[0]) {
    if (NT) __builtin_nontemporal_store(res[0], out + row0);
    else out[row0] = res[0];
  }
}

// Workgroups are dealt round-robin over the 8 XCDs (b and b + 8 share an L2).  A banded
// operator re-reads x at +-(half-bandwidth) rows, i.e. a few tiles away, so every XCD
// gets ONE contiguous run of tiles: the re-reads then hit the L2 that fetched the line
// (measured on level 1 of the 4096^2 hierarchy: x fetched 2.1x -> see DESIGN.md).
// on >= 16: a WIDE band (3-D levels: x is re-read a whole grid plane = `on` tiles away, far beyond
// what an L2 keeps of a contiguous run).  Every XCD then takes the same slab of on / 8 tiles out of
// EVERY plane, plane after plane: the +-plane re-reads come back after one slab (a few hundred KB)
// of the XCD's own traffic, the +-line ones sit inside the slab.
__device__ __forceinline__ int xcd_tile(unsigned b, unsigned nb, int on) {
  if (!on) return (int)b;
  if (on >= 16) {
    const unsigned tp = (unsigned)on, s = tp >> 3;
    if (b >= nb / tp * tp) return (int)b;  // the last, partial plane: plain order
    const unsigned k = b & 7u, i = b >> 3, p = i / s;
    return (int)(p * tp + k * s + (i - p * s));
  }
  const unsigned k = b & 7u, i = b >> 3, q = nb >> 3, r = nb & 7u;
  return (int)(k * q + (k < r ? k : r) + i);
}
// (Two tiles per workgroup, i.e. the streamed operands of twice as many rows in flight per
// lane, measured SLOWER on the 4096^2 fine level: 99.5 vs 86.8 us, 90 VGPRs.)
template <int MODE, int WORDS, int UN, bool NT, int R>
__global__ __launch_bounds__(256) void dict_kernel(
    int n, const uint64_t* __restrict__ codes, const uint8_t* __restrict__ rtype,
    const uint64_t* __restrict__ rwords, const int32_t* __restrict__ doff,
    const double* __restrict__ dval, int ntab, const double* x, const double* __restrict__ f,
    double* out, double omega, int dshift, int xcd_map, const double* __restrict__ utd,
    const int32_t* __restrict__ uti, double* dvec, double alpha) {
  __shared__ DictEntry tab[256];
  __shared__ uint64_t wtab[256 * WORDS];
  const int row0 = (xcd_tile(blockIdx.x, gridDim.x, xcd_map) * 256 + (int)threadIdx.x) * R;
  DictStream<WORDS, R> s;
  dict_fetch<MODE, WORDS, NT, R>(s, row0, n, codes, rtype, f, x, dshift, dvec);  // in flight while the tables are staged
  dict_stage_table<MODE>(tab, doff, dval, ntab);
  if (rtype) dict_stage_words<WORDS>(wtab, rwords);
  __syncthreads();
  double res[R];
  bool fast = false;
  if constexpr ((mode_jac(MODE) || MODE == CSR_RESID) && R == 2 && (UN == 7 || UN == 16)) {
    if (utd) fast = dict_stencil_can<UN>(s.ty, s.live, uti);
    if (fast) dict_rows_stencil<MODE, UN>(s.ty, s.fi, s.xi, row0, utd, uti, x, omega, res);
  }
  if (!fast) {
    if (rtype) dict_expand<WORDS, R>(s, wtab);
    dict_rows<MODE, WORDS, UN, R>(s, row0, tab, x, omega, dshift, res);
  }
  if constexpr (mode_cheb(MODE)) {  // res = t_i
    double dn[R];
#pragma unroll
    for (int r = 0; r < R; ++r) res[r] = cheb_update<MODE>(res[r], s.xi[r], s.di[r], alpha, omega, dn[r]);
    if (!cheb_last(MODE)) dict_store<WORDS, NT, R>(s, row0, dn, dvec);
  }
  dict_store<WORDS, NT, R>(s, row0, res, out);
}

// ---- fused forms for the true-Jacobi V-cycle on linear-interpolation levels --------
// Tiles of 256 R rows that OVERLAP by two rows (stride 256 R - 2): the row results of
// a tile are parked in LDS, and everything a coarse point j needs from the fine rows
// 2j, 2j+1, 2j+2 (restriction) or from its neighbour j-1 (prolongation) is then inside
// one tile.  The two duplicated rows are recomputed (0.4 %) and stored twice with the
// same bits.  Same per-row arithmetic and the same transfer expressions as the
// separate kernels, so the V-cycle is bit-identical with and without these fusions.
//
// (1) residual + restriction + first coarse Jacobi sweep (multigrid.hpp:272-282, then
// :268 on level l+1 whose u is zero): r = f - A u is written, f_H = R r is written, and
// the from-zero sweep of the coarse level (jacobi_from_zero_kernel) is written to uH1.
// Other smoothers (uH1 == nullptr): the coarse u is zero-filled instead (uH0, :278).
// restriction of a tile's residuals rs[0 .. 256 R) (rows tile * (256 R - 2) ...) and, when
// uH1 is given, the first coarse Jacobi sweep from zero; else the coarse u is zero-filled
template <int R>
__device__ __forceinline__ void dict_restrict_tail(int tile, int n, const double* rs, int nH,
                                                   double* __restrict__ fH,
                                                   const double* __restrict__ diagH,
                                                   double* __restrict__ uH1,
                                                   double* __restrict__ uH0, double omega) {
  for (int q = threadIdx.x; q < 128 * R - 1; q += 256) {
    const int j = tile * (128 * R - 1) + q;
    if (j >= nH) break;
    const int64_t i = 2 * (int64_t)j;  // linear_restrict_kernel, same guards and order
    double sum = 0.0;
    if (i < n) sum += 0.5 * rs[2 * q];
    if (i + 1 < n) sum += 1.0 * rs[2 * q + 1];
    if (i + 2 < n) sum += 0.5 * rs[2 * q + 2];
    fH[j] = sum;
    if (uH1) {
      const double xi = 0.0, acc = 0.0;  // jacobi_from_zero_kernel
      const double d = diagH[j];
      uH1[j] = (d == 0.0) ? xi : xi + omega * ((sum - acc) / d - xi);
    } else {
      uH0[j] = 0.0;  // multigrid.hpp:278
    }
  }
}
// prolongation of a tile's new coarse values rs[] into the finer level:
// uh_out[2j] = uh_in[2j] + (0.5 u_H[j-1] + 0.5 u_H[j]), uh_out[2j+1] = uh_in[2j+1] + u_H[j]
// (linear_prolong_add2_kernel).  The tile prolongs the coarse points q = 1 .. stride (q = 0
// too in the first tile); j = n is the virtual point whose fine rows only receive the left
// neighbour / + 0.0.  uh_in == uh_out is the in-place form.
template <int R>
__device__ __forceinline__ void dict_prolong_tail(int tile, int n, const double* rs, int n_h,
                                                  const double* uh_in, double* uh_out) {
  typedef double f64x2 __attribute__((ext_vector_type(2)));
  const int stride = 256 * R - 2;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int q = (int)threadIdx.x * R + r;
    const int j = tile * stride + q;
    if ((q == 0 && tile != 0) || q > stride || j > n) continue;
    double t0 = 0.0, t1 = 0.0;
    const double b = (j < n) ? rs[q] : 0.0;
    if (j >= 1 && j - 1 < n) t0 += 0.5 * rs[q - 1];
    if (j < n) {
      t0 += 0.5 * b;
      t1 += 1.0 * b;
    }
    const int64_t i = 2 * (int64_t)j;
    if (i + 1 < n_h) {
      f64x2 u = *reinterpret_cast<const f64x2*>(uh_in + i);
      u.x = u.x + t0;
      u.y = u.y + t1;
      *reinterpret_cast<f64x2*>(uh_out + i) = u;
    } else if (i < n_h) {
      uh_out[i] = uh_in[i] + t0;
    }
  }
}
// The same two tails with their global operand already in registers (the pair kernels issue
// every load at kernel entry): *_pre is the load, under the guards of the tail that uses it.
// R = 2: a lane owns one coarse row of the restriction, two coarse points of the prolongation.
__device__ __forceinline__ double dict_restrict_pre(int tile, int nH, const double* __restrict__ diagH) {
  const int q = threadIdx.x, j = tile * 255 + q;
  return (q < 255 && j < nH) ? diagH[j] : 0.0;
}
__device__ __forceinline__ void dict_restrict_tail(int tile, int n, const double* rs, int nH,
                                                   double* __restrict__ fH, double dH,
                                                   double* __restrict__ uH1, double omega) {
  const int q = threadIdx.x, j = tile * 255 + q;
  if (q >= 255 || j >= nH) return;
  const int64_t i = 2 * (int64_t)j;  // linear_restrict_kernel, same guards and order
  double sum = 0.0;
  if (i < n) sum += 0.5 * rs[2 * q];
  if (i + 1 < n) sum += 1.0 * rs[2 * q + 1];
  if (i + 2 < n) sum += 0.5 * rs[2 * q + 2];
  fH[j] = sum;
  const double xi = 0.0, acc = 0.0;  // jacobi_from_zero_kernel
  const double d = dH;
  uH1[j] = (d == 0.0) ? xi : xi + omega * ((sum - acc) / d - xi);
}
typedef double pair_f64x2 __attribute__((ext_vector_type(2)));
// (lone: the last entry of uh_in when n_h is odd -- at most one of a lane's two coarse points has
// it -- in a register of its own: loaded into pre[r].x, the two forms share registers and the
// compiler drains every load in flight between them)
// (STRIDE: rows a tile advances by; the pair kernels' 510, K-Duo also runs shorter tiles)
template <int STRIDE = 510>
__device__ __forceinline__ void dict_prolong_pre(int tile, int n, int n_h, const double* uh_in,
                                                 pair_f64x2 (&pre)[2], double& lone) {
  bool two[2], one[2];
  int64_t i[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int q = (int)threadIdx.x * 2 + r;
    const int j = tile * STRIDE + q;
    const bool on = !((q == 0 && tile != 0) || q > STRIDE || j > n);
    i[r] = 2 * (int64_t)j;
    two[r] = on && i[r] + 1 < n_h;
    one[r] = on && i[r] + 1 == n_h;
    pre[r].x = pre[r].y = 0.0;
  }
  lone = 0.0;
#pragma unroll
  for (int r = 0; r < 2; ++r)
    if (two[r]) pre[r] = *reinterpret_cast<const pair_f64x2*>(uh_in + i[r]);
  if (one[0] || one[1]) lone = uh_in[n_h - 1];
}
template <int STRIDE = 510>
__device__ __forceinline__ void dict_prolong_tail(int tile, int n, const double* rs, int n_h,
                                                  const pair_f64x2 (&pre)[2], double lone,
                                                  double* uh_out) {
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int q = (int)threadIdx.x * 2 + r;
    const int j = tile * STRIDE + q;
    if ((q == 0 && tile != 0) || q > STRIDE || j > n) continue;
    double t0 = 0.0, t1 = 0.0;
    const double b = (j < n) ? rs[q] : 0.0;
    if (j >= 1 && j - 1 < n) t0 += 0.5 * rs[q - 1];
    if (j < n) {
      t0 += 0.5 * b;
      t1 += 1.0 * b;
    }
    const int64_t i = 2 * (int64_t)j;
    if (i + 1 < n_h) {
      pair_f64x2 u = pre[r];
      u.x = u.x + t0;
      u.y = u.y + t1;
      *reinterpret_cast<pair_f64x2*>(uh_out + i) = u;
    } else if (i < n_h) {
      uh_out[i] = lone + t0;
    }
  }
}
template <int WORDS, int UN, bool NT, int R>
__global__ __launch_bounds__(256) void dict_resid_restrict_kernel(
    int n, const uint64_t* __restrict__ codes, const uint8_t* __restrict__ rtype,
    const uint64_t* __restrict__ rwords, const int32_t* __restrict__ doff,
    const double* __restrict__ dval, int ntab, const double* x, const double* __restrict__ f,
    double* r_out, int nH, double* __restrict__ fH, const double* __restrict__ diagH,
    double* __restrict__ uH1, double* __restrict__ uH0, double omega, int xcd_map,
    const double* __restrict__ utd, const int32_t* __restrict__ uti) {
  __shared__ DictEntry tab[256];
  __shared__ uint64_t wtab[256 * WORDS];
  __shared__ double rs[256 * R];
  const int tile = xcd_tile(blockIdx.x, gridDim.x, xcd_map);
  const int row0 = tile * (256 * R - 2) + (int)threadIdx.x * R;
  DictStream<WORDS, R> s;
  dict_fetch<CSR_RESID, WORDS, NT, R>(s, row0, n, codes, rtype, f, x, 0);
  dict_stage_table<CSR_RESID>(tab, doff, dval, ntab);
  if (rtype) dict_stage_words<WORDS>(wtab, rwords);
  __syncthreads();
  double res[R];
  bool fast = false;
  if constexpr (R == 2 && (UN == 7 || UN == 16)) {
    if (utd) fast = dict_stencil_can<UN>(s.ty, s.live, uti);
    if (fast) dict_rows_stencil<CSR_RESID, UN>(s.ty, s.fi, s.xi, row0, utd, uti, x, omega, res);
  }
  if (!fast) {
    if (rtype) dict_expand<WORDS, R>(s, wtab);
    dict_rows<CSR_RESID, WORDS, UN, R>(s, row0, tab, x, omega, 0, res);
  }
  if (r_out) dict_store<WORDS, NT, R>(s, row0, res, r_out);  // nullptr: r is dead after this kernel
#pragma unroll
  for (int r = 0; r < R; ++r) rs[threadIdx.x * R + r] = s.live[r] ? res[r] : 0.0;
  __syncthreads();
  dict_restrict_tail<R>(tile, n, rs, nH, fH, diagH, uH1, uH0, omega);
}
// (2) Jacobi sweep on level H + prolongation of its result into the finer level
// (multigrid.hpp:300 on level l+1, then :294-296 on level l):
// u_h[2j] += 0.5 u_H[j-1] + 0.5 u_H[j], u_h[2j+1] += u_H[j] (linear_prolong_add2_kernel).
template <int WORDS, int UN, bool NT, int R>
__global__ __launch_bounds__(256) void dict_jacobi_prolong_kernel(
    int n, const uint64_t* __restrict__ codes, const uint8_t* __restrict__ rtype,
    const uint64_t* __restrict__ rwords, const int32_t* __restrict__ doff,
    const double* __restrict__ dval, int ntab, const double* x, const double* __restrict__ f,
    double* out, double omega, int n_h, const double* uh_in, double* uh_out, int xcd_map,
    const double* __restrict__ utd, const int32_t* __restrict__ uti) {
  __shared__ DictEntry tab[256];
  __shared__ uint64_t wtab[256 * WORDS];
  __shared__ double rs[256 * R];
  const int tile = xcd_tile(blockIdx.x, gridDim.x, xcd_map);
  const int stride = 256 * R - 2;
  const int row0 = tile * stride + (int)threadIdx.x * R;
  DictStream<WORDS, R> s;
  dict_fetch<CSR_JACOBI, WORDS, NT, R>(s, row0, n, codes, rtype, f, x, 0);
  dict_stage_table<CSR_JACOBI>(tab, doff, dval, ntab);
  if (rtype) dict_stage_words<WORDS>(wtab, rwords);
  __syncthreads();
  double res[R];
  bool fast = false;
  if constexpr (R == 2 && (UN == 7 || UN == 16)) {
    if (utd) fast = dict_stencil_can<UN>(s.ty, s.live, uti);
    if (fast) dict_rows_stencil<CSR_JACOBI, UN>(s.ty, s.fi, s.xi, row0, utd, uti, x, omega, res);
  }
  if (!fast) {
    if (rtype) dict_expand<WORDS, R>(s, wtab);
    dict_rows<CSR_JACOBI, WORDS, UN, R>(s, row0, tab, x, omega, 0, res);
  }
  dict_store<WORDS, NT, R>(s, row0, res, out);
#pragma unroll
  for (int r = 0; r < R; ++r) rs[threadIdx.x * R + r] = s.live[r] ? res[r] : 0.0;
  __syncthreads();
  dict_prolong_tail<R>(tile, n, rs, n_h, uh_in, uh_out);
}

// ---- two sweeps in one launch on small levels ----------------------------------------
// Below ~300 K rows a launch costs more than its work (~5 us each), and the band is narrow
// (half-bandwidth hb <= 64 rows).  A tile then computes its first Jacobi sweep on its rows
// PLUS hb rows on either side (recomputed by the neighbouring tiles, <= 25 %) into an LDS
// window, and the operation that follows reads its x from that window:
//   down: sweep + (residual + restriction + first coarse sweep)   [dict_pair_down_kernel]
//   up:   sweep + (sweep + prolongation into the finer level)     [dict_pair_up_kernel]
// Same row arithmetic (dict_rows) and the same tails, so the V-cycle stays bit-identical.
// R = 2 rows per lane, plain loads/stores.  w0 = tile start - hbw (hbw even >= hb).
//
// Memory phase.  Every operand of a tile is known at kernel entry, so the workgroup issues ALL its
// global loads there, waits once, and afterwards touches global memory only to store:
//   the table entries, the window of `a` the first sweep gathers from (rows [w0 - hbw,
//   w0 + W + hbw), W = 512 + 2 hbw; 0.0 outside the matrix), f and the row types (or the code
//   words) of the W window rows -> LDS;  the operand of the tail (coarse diagonal / the fine u
//   the prolongation adds to) -> registers.
// Both sweeps then gather from LDS (aw, then uw) and read f / types / codes from LDS: one global
// round trip per launch on levels whose work is a few microseconds (gathering the first sweep from
// global memory behind the staged tables, fetching f and the types per step and loading the tail's
// operand at the end were five to seven dependent ones: DESIGN.md section 4).
constexpr int PAIR_HB = 66;                       // largest half-window, in rows
constexpr int PAIR_W = 512 + 2 * PAIR_HB;         // window capacity: rows the first sweep forms
constexpr int PAIR_AW = PAIR_W + 2 * PAIR_HB;     // rows of `a` under them
constexpr int PAIR_AP = (PAIR_AW / 2 + 255) / 256;  // passes of 256 lanes x 2 rows over aw
static_assert(PAIR_W <= 1024 && PAIR_HB % 2 == 0, "two passes of 512 rows cover the window");

typedef uint64_t pair_u64x2 __attribute__((ext_vector_type(2)));
// What one lane has in flight between kernel entry and the first barrier.  The loads land in
// registers that nothing writes again before the commit (defaults first, then the loads under
// their guards), so that no wait sits between two loads.
template <int WORDS>
struct PairLoads {
  double tv;        // table entry threadIdx.x
  int32_t to;
  uint64_t rw[WORDS];
  pair_f64x2 a[PAIR_AP];       // rows w0 - hbw + 2 (k 256 + t), + 1 of a
  // window rows 2 (k 256 + t), + 1: f, the two row types or the code words (words 2 j, 2 j + 1 of
  // the 2 WORDS).  *l: the same for the matrix's last row when it has no partner.
  pair_f64x2 f[2];
  double fl[2];
  uint32_t ty[2], tl[2];
  pair_u64x2 c[2][WORDS], cl[2];
};
// TYPES: the matrix has row types (the caller branches once, so that each form is straight code
// and leaves the other form's registers alone).
template <int WORDS, bool TYPES>
__device__ __forceinline__ void dict_pair_issue(PairLoads<WORDS>& g, int n, int w0, int hbw,
                                                const uint64_t* __restrict__ codes,
                                                const uint8_t* __restrict__ rtype,
                                                const uint64_t* __restrict__ rwords,
                                                const int32_t* __restrict__ doff,
                                                const double* __restrict__ dval, int ntab,
                                                const double* a, const double* __restrict__ f) {
  const int t = threadIdx.x;
  const int W = 512 + 2 * hbw, AW = W + 2 * hbw;
  g.tv = t < ntab ? dval[t] : 0.0;
  g.to = t < ntab ? doff[t] : 0;
#pragma unroll
  for (int k = 0; k < WORDS; ++k) g.rw[k] = TYPES ? rwords[t * WORDS + k] : 0;
#pragma unroll
  for (int k = 0; k < PAIR_AP; ++k) {
    const int idx = (k * 256 + t) * 2;
    const int row = w0 - hbw + idx;  // even: a pair is either entirely before row 0 or not at all
    g.a[k].x = g.a[k].y = 0.0;
    if (idx < AW && row >= 0) {
      if (row + 1 < n) g.a[k] = *reinterpret_cast<const pair_f64x2*>(a + row);
      else if (row < n) g.a[k].x = a[row];
    }
  }
  // rows before the matrix (first tile), past it or past the window: empty rows, no loads
  bool both[2], lone[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int lw = (k * 256 + t) * 2, row0 = w0 + lw;
    const bool inside = row0 >= 0 && lw < W;
    both[k] = inside && row0 + 1 < n;
    lone[k] = inside && row0 + 1 == n;
    g.f[k].x = g.f[k].y = g.fl[k] = 0.0;
    if (both[k]) g.f[k] = *reinterpret_cast<const pair_f64x2*>(f + row0);
    if (lone[k]) g.fl[k] = f[row0];
  }
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int row0 = w0 + (k * 256 + t) * 2;
    if (TYPES) {
      g.ty[k] = 0xFFFFu;
      g.tl[k] = 0xFFu;
      if (both[k]) g.ty[k] = *reinterpret_cast<const uint16_t*>(rtype + row0);
      if (lone[k]) g.tl[k] = rtype[row0];
    } else {
      g.cl[k].x = g.cl[k].y = ~(uint64_t)0;
#pragma unroll
      for (int j = 0; j < WORDS; ++j) g.c[k][j].x = g.c[k][j].y = ~(uint64_t)0;
      const uint64_t* cp = codes + (int64_t)row0 * WORDS;
      if (both[k]) {
#pragma unroll
        for (int j = 0; j < WORDS; ++j) g.c[k][j] = reinterpret_cast<const pair_u64x2*>(cp)[j];
      }
      if (lone[k]) {
        if (WORDS == 2) g.cl[k] = *reinterpret_cast<const pair_u64x2*>(cp);
        else g.cl[k].x = cp[0];
      }
    }
  }
}
// wc: the word table of the row types when the matrix has them, else the code words of the window
template <int WORDS, bool TYPES>
__device__ __forceinline__ void dict_pair_commit(const PairLoads<WORDS>& g, int n, int w0, int hbw,
                                                 uint64_t* wc, uint16_t* tw, double* aw,
                                                 double* fw) {
  const int t = threadIdx.x;
  const int W = 512 + 2 * hbw, AW = W + 2 * hbw;
  if (TYPES) {
#pragma unroll
    for (int k = 0; k < WORDS; ++k) wc[t * WORDS + k] = g.rw[k];
  }
#pragma unroll
  for (int k = 0; k < PAIR_AP; ++k) {
    const int idx = (k * 256 + t) * 2;
    if (idx < AW) *reinterpret_cast<pair_f64x2*>(aw + idx) = g.a[k];
  }
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int lw = (k * 256 + t) * 2;
    if (lw >= W) continue;
    const bool both = w0 + lw >= 0 && w0 + lw + 1 < n;  // else: the lone last row, or no row at all
    pair_f64x2 fv = g.f[k];
    fv.x = both ? fv.x : g.fl[k];
    *reinterpret_cast<pair_f64x2*>(fw + lw) = fv;
    if (TYPES) {
      // (the empty asm keeps the OR here: formed right behind its load, in the one wave that holds
      // the matrix's last row, it would put a wait between the loads.  That rests on the compiler's
      // scheduling -- ROCm 7.2, AMD clang 22 -- and tools/pair_loads_check.py shows it in the assembly.)
      uint32_t tl = g.tl[k];
      asm volatile("" : "+v"(tl));
      tw[lw >> 1] = (uint16_t)(both ? g.ty[k] : (tl | 0xFF00u));
    } else {
      pair_u64x2* wp = reinterpret_cast<pair_u64x2*>(wc + lw * WORDS);
      wp[0] = both ? g.c[k][0] : g.cl[k];
      if (WORDS == 2) wp[1] = g.c[k][WORDS - 1];
    }
  }
}
// the stream of window rows lw, lw + 1 (matrix rows row0, row0 + 1) from LDS; xi is the caller's
template <int WORDS>
__device__ __forceinline__ void dict_pair_stream(DictStream<WORDS, 2>& s, int lw, int W, int row0, int n,
                                                 bool types, const uint64_t* wc, const uint16_t* tw,
                                                 const double* fw) {
  const bool inside = row0 >= 0 && lw < W;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    s.live[r] = inside && row0 + r < n;
    s.cw[r][0] = s.cw[r][1] = ~(uint64_t)0;
    s.fi[r] = s.xi[r] = s.di[r] = 0.0;
  }
  s.ty = 0xFFFFu;
  if (lw < W) {  // rows outside the matrix were committed as empty rows
    const pair_f64x2 fv = *reinterpret_cast<const pair_f64x2*>(fw + lw);
    s.fi[0] = fv.x; s.fi[1] = fv.y;
    if (types) {
      s.ty = tw[lw >> 1];
    } else {
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int j = 0; j < WORDS; ++j) s.cw[r][j] = wc[(lw + r) * WORDS + j];
    }
  }
}

// first stage: Jacobi sweep of the window rows [w0, w0 + 512 + 2 hbw) from the LDS copy of `a`
// (aw[i] = a[w0 - hbw + i]) into uw (0.0 for rows outside the matrix); rows of the tile are also
// stored to u_out if given.  A row that is not live has all codes 0xFF: it gathers aw[0].
template <int WORDS, int UN>
__device__ __forceinline__ void dict_pair_stage1(int n, int w0, int hbw, bool types,
                                                 const DictEntry* tabJ, const uint64_t* wc,
                                                 const uint16_t* tw, const double* aw,
                                                 const double* fw, double omega, double* uw,
                                                 double* u_out) {
  const int W = 512 + 2 * hbw;
  for (int base = 0; base < W; base += 512) {  // 2 passes, the second one over the 2 hbw rows left
    const int lw = base + (int)threadIdx.x * 2;  // index in the window
    const int row0 = w0 + lw;
    DictStream<WORDS, 2> s;
    dict_pair_stream<WORDS>(s, lw, W, row0, n, types, wc, tw, fw);
    if (lw < W) {
      s.xi[0] = aw[lw + hbw];
      s.xi[1] = aw[lw + hbw + 1];
    }
    if (types) dict_expand<WORDS, 2>(s, wc);
    double res[2];
    dict_rows<CSR_JACOBI, WORDS, UN, 2>(s, lw + hbw, tabJ, aw, omega, 0, res);
    if (lw < W) {
      uw[lw] = s.live[0] ? res[0] : 0.0;
      uw[lw + 1] = s.live[1] ? res[1] : 0.0;
    }
    if (u_out && lw >= hbw && lw < hbw + 512) dict_store<WORDS, false, 2>(s, row0, res, u_out);
  }
}
template <int WORDS, int UN>
__global__ __launch_bounds__(256) void dict_pair_down_kernel(
    int n, const uint64_t* __restrict__ codes, const uint8_t* __restrict__ rtype,
    const uint64_t* __restrict__ rwords, const int32_t* __restrict__ doff,
    const double* __restrict__ dval, int ntab, const double* a, const double* __restrict__ f,
    double* u_out, double* r_out, int nH, double* __restrict__ fH,
    const double* __restrict__ diagH, double* __restrict__ uH1, double omega, int hbw,
    int xcd_map) {
  __shared__ DictEntry tabJ[256];
  __shared__ DictEntry tabR[256];
  __shared__ __attribute__((aligned(16))) uint64_t wc[PAIR_W * WORDS];
  __shared__ uint16_t tw[PAIR_W / 2];
  __shared__ __attribute__((aligned(16))) double aw[PAIR_AW];
  __shared__ __attribute__((aligned(16))) double fw[PAIR_W];
  __shared__ double uw[PAIR_W];
  __shared__ double rs[512];
  const int tile = xcd_tile(blockIdx.x, gridDim.x, xcd_map);
  const int t0 = tile * 510, w0 = t0 - hbw, W = 512 + 2 * hbw;
  const bool types = rtype != nullptr;
  PairLoads<WORDS> g;
  if (types) dict_pair_issue<WORDS, true>(g, n, w0, hbw, codes, rtype, rwords, doff, dval, ntab, a, f);
  else dict_pair_issue<WORDS, false>(g, n, w0, hbw, codes, rtype, rwords, doff, dval, ntab, a, f);
  const double dH = dict_restrict_pre(tile, nH, diagH);
  dict_put_table<CSR_JACOBI>(tabJ, g.tv, g.to, ntab);
  dict_put_table<CSR_RESID>(tabR, g.tv, g.to, ntab);
  if (types) dict_pair_commit<WORDS, true>(g, n, w0, hbw, wc, tw, aw, fw);
  else dict_pair_commit<WORDS, false>(g, n, w0, hbw, wc, tw, aw, fw);
  __syncthreads();
  dict_pair_stage1<WORDS, UN>(n, w0, hbw, types, tabJ, wc, tw, aw, fw, omega, uw, u_out);
  __syncthreads();
  const int row0 = t0 + (int)threadIdx.x * 2;
  DictStream<WORDS, 2> s;
  dict_pair_stream<WORDS>(s, row0 - w0, W, row0, n, types, wc, tw, fw);
  if (types) dict_expand<WORDS, 2>(s, wc);
  double res[2];
  dict_rows<CSR_RESID, WORDS, UN, 2>(s, row0 - w0, tabR, uw, omega, 0, res);  // x = the LDS window
  if (r_out) dict_store<WORDS, false, 2>(s, row0, res, r_out);
  rs[threadIdx.x * 2] = s.live[0] ? res[0] : 0.0;
  rs[threadIdx.x * 2 + 1] = s.live[1] ? res[1] : 0.0;
  __syncthreads();
  dict_restrict_tail(tile, n, rs, nH, fH, dH, uH1, omega);
}
template <int WORDS, int UN>
__global__ __launch_bounds__(256) void dict_pair_up_kernel(
    int n, const uint64_t* __restrict__ codes, const uint8_t* __restrict__ rtype,
    const uint64_t* __restrict__ rwords, const int32_t* __restrict__ doff,
    const double* __restrict__ dval, int ntab, const double* a, const double* __restrict__ f,
    double* u_out, double omega, int hbw, int n_h, const double* uh_in, double* uh_out,
    int xcd_map) {
  __shared__ DictEntry tabJ[256];
  __shared__ __attribute__((aligned(16))) uint64_t wc[PAIR_W * WORDS];
  __shared__ uint16_t tw[PAIR_W / 2];
  __shared__ __attribute__((aligned(16))) double aw[PAIR_AW];
  __shared__ __attribute__((aligned(16))) double fw[PAIR_W];
  __shared__ double uw[PAIR_W];
  __shared__ double rs[512];
  const int tile = xcd_tile(blockIdx.x, gridDim.x, xcd_map);
  const int t0 = tile * 510, w0 = t0 - hbw, W = 512 + 2 * hbw;
  const bool types = rtype != nullptr;
  PairLoads<WORDS> g;
  if (types) dict_pair_issue<WORDS, true>(g, n, w0, hbw, codes, rtype, rwords, doff, dval, ntab, a, f);
  else dict_pair_issue<WORDS, false>(g, n, w0, hbw, codes, rtype, rwords, doff, dval, ntab, a, f);
  pair_f64x2 pre[2];  // uh_in may be uh_out: a lane reads only the rows it later writes
  double pre1;        // the lone last entry
  dict_prolong_pre(tile, n, n_h, uh_in, pre, pre1);
  dict_put_table<CSR_JACOBI>(tabJ, g.tv, g.to, ntab);
  if (types) dict_pair_commit<WORDS, true>(g, n, w0, hbw, wc, tw, aw, fw);
  else dict_pair_commit<WORDS, false>(g, n, w0, hbw, wc, tw, aw, fw);
  __syncthreads();
  dict_pair_stage1<WORDS, UN>(n, w0, hbw, types, tabJ, wc, tw, aw, fw, omega, uw, nullptr);
  __syncthreads();
  const int row0 = t0 + (int)threadIdx.x * 2;
  DictStream<WORDS, 2> s;
  dict_pair_stream<WORDS>(s, row0 - w0, W, row0, n, types, wc, tw, fw);
  s.xi[0] = uw[row0 - w0];
  s.xi[1] = uw[row0 - w0 + 1];
  if (types) dict_expand<WORDS, 2>(s, wc);
  double res[2];
  dict_rows<CSR_JACOBI, WORDS, UN, 2>(s, row0 - w0, tabJ, uw, omega, 0, res);
  dict_store<WORDS, false, 2>(s, row0, res, u_out);
  rs[threadIdx.x * 2] = s.live[0] ? res[0] : 0.0;
  rs[threadIdx.x * 2 + 1] = s.live[1] ? res[1] : 0.0;
  __syncthreads();
  dict_prolong_tail(tile, n, rs, n_h, pre, pre1, uh_out);
}

// ---- K-Duo: two consecutive pair levels in one launch ---------------------------------------
// The pair launches of the levels 6+ of the 4096^2 hierarchy sit within 2 us of the cost of an empty
// launch, so one more step of the same kind: the down-legs of levels (l, l+1), or the up-legs of
// (l+1, l), as ONE plain launch of independent workgroups.  A tile owns T rows of level l (DUO_T or
// DUO_T_SMALL), the level-(l+1) rows c with 2c in it and the level-(l+2) rows cc with 4cc in it; everything
// else it needs is recomputed from a wider window of the loaded operands (duo_windows: the
// dependencies walked backwards).  All global loads are issued at entry and committed with one wait
// (DuoLoads / duo_issue / duo_commit: PairLoads with the windows as arguments); every row comes from
// dict_rows on LDS windows and the transfers are the expressions of dict_restrict_tail,
// jacobi_from_zero_kernel, linear_prolong_add2_kernel and dict_prolong_tail, so a duo leaves the bits
// of the four pair launches it replaces.  One DictEntry table serves both levels and both modes in
// turn (rewritten from registers behind a barrier): the LDS stays below 64 KB.
//
// Windows.  hbw0 / hbw1: the even half-windows of levels l / l+1.  Level-(l+1) windows are given from
// ce = (t0 / 2) & ~1 (t0 = the tile's first row: even, so that pairs never straddle an end), level-l
// windows of the down-leg from 2 ce, those of the up-leg from t0: window = [base - lo, base - lo + count).
enum {
  DW_D_R1_LO, DW_D_R1,  // down: residual of l+1 (owned rows + 2)
  DW_D_U1_LO, DW_D_U1,  //       second sweep of l+1
  DW_D_M1_LO, DW_D_M1,  //       f_{l+1} and its first sweep from zero
  DW_D_R0_LO, DW_D_R0,  //       residual of l
  DW_D_M0_LO, DW_D_M0,  //       second sweep of l (f, row types)
  DW_D_A0_LO, DW_D_A0,  //       tmp_l under it
  DW_U_S1_LO, DW_U_S1,  // up:   second sweep of l+1
  DW_U_M1_LO, DW_U_M1,  //       first sweep of l+1 (f, row types)
  DW_U_A1_LO, DW_U_A1,  //       tmp_{l+1} under it
  DW_U_S0_LO, DW_U_S0,  //       second sweep of l (the frame of the prolongation: tile + 2)
  DW_U_M0_LO, DW_U_M0,  //       first sweep of l
  DW_U_A0_LO, DW_U_A0,  //       u_l + P u_{l+1}
  DW_CAP_D_M1, DW_CAP_D_M0, DW_CAP_D_A0, DW_CAP_U_M1, DW_CAP_U_A1, DW_CAP_U_M0, DW_CAP_U_A0,
  DW_COUNT
};
// Rows of level l a tile owns: the pair kernels' 510 under a wide band; 254 where the halo is small
// against the tile (half-window of level l <= DUO_T_SMALL_HBW), so that every window is one pass of
// 256 lanes x 2 rows and twice as many workgroups share the work.  A duo's time is the chain of its
// dependent passes, not its rows.
constexpr int DUO_T = 510;
constexpr int DUO_T_SMALL = 254;
constexpr int DUO_T_SMALL_HBW = 34;
constexpr int DUO_D_M1 = 448;                         // capacities, in rows
constexpr int DUO_D_M0 = 1024;
constexpr int DUO_D_A0 = DUO_D_M0 + 2 * PAIR_HB;
constexpr int DUO_U_M1 = 512;
constexpr int DUO_U_A1 = DUO_U_M1 + 2 * PAIR_HB;
constexpr int DUO_U_M0 = 512 + 2 * PAIR_HB;
constexpr int DUO_U_A0 = DUO_U_M0 + 2 * PAIR_HB;
static_assert(DW_COUNT == AMG_DUO_WINDOWS_LEN, "kernels.hpp");
__host__ __device__ inline void duo_windows(int hbw0, int hbw1, int T, int* w) {
  const int r1 = (T / 2 + 4) & ~1;  // owned c + 2, + 1 for an odd t0 / 2
  w[DW_D_R1_LO] = 0;                    w[DW_D_R1] = r1;
  w[DW_D_U1_LO] = hbw1;                 w[DW_D_U1] = r1 + 2 * hbw1;
  w[DW_D_M1_LO] = 2 * hbw1;             w[DW_D_M1] = r1 + 4 * hbw1;
  w[DW_D_R0_LO] = 4 * hbw1;             w[DW_D_R0] = 2 * w[DW_D_M1] + 2;  // rows 2c .. 2c + 2
  w[DW_D_M0_LO] = 4 * hbw1 + hbw0;      w[DW_D_M0] = w[DW_D_R0] + 2 * hbw0;
  w[DW_D_A0_LO] = 4 * hbw1 + 2 * hbw0;  w[DW_D_A0] = w[DW_D_R0] + 4 * hbw0;
  const int s0 = T + 2;
  w[DW_U_S0_LO] = 0;         w[DW_U_S0] = s0;
  w[DW_U_M0_LO] = hbw0;      w[DW_U_M0] = s0 + 2 * hbw0;
  w[DW_U_A0_LO] = 2 * hbw0;  w[DW_U_A0] = s0 + 4 * hbw0;
  // fine row i takes u_{l+1}[i / 2 - 1 .. i / 2] (even i) or [i / 2] (odd i)
  const int s1 = (s0 / 2 + 2 * hbw0 + 4) & ~1;
  w[DW_U_S1_LO] = hbw0 + 2;             w[DW_U_S1] = s1;
  w[DW_U_M1_LO] = hbw0 + 2 + hbw1;      w[DW_U_M1] = s1 + 2 * hbw1;
  w[DW_U_A1_LO] = hbw0 + 2 + 2 * hbw1;  w[DW_U_A1] = s1 + 4 * hbw1;
  w[DW_CAP_D_M1] = DUO_D_M1; w[DW_CAP_D_M0] = DUO_D_M0; w[DW_CAP_D_A0] = DUO_D_A0;
  w[DW_CAP_U_M1] = DUO_U_M1; w[DW_CAP_U_A1] = DUO_U_A1; w[DW_CAP_U_M0] = DUO_U_M0; w[DW_CAP_U_A0] = DUO_U_A0;
}

// What the tile that starts at row t0 of level l owns: rows [o[0], o[1]) of level l, the rows c of
// level l+1 with 2c among them = [o[2], o[3]), the rows cc of level l+2 with 4cc among them =
// [o[4], o[5]) -- before clipping to the levels' sizes.  t0 and T are even.
__host__ __device__ inline void duo_owned(int t0, int T, int* o) {
  o[0] = t0;             o[1] = t0 + T;
  o[2] = t0 / 2;         o[3] = (t0 + T) / 2;
  o[4] = (t0 + 3) >> 2;  o[5] = (t0 + T + 3) >> 2;
}
// PairLoads with the windows as arguments: AP passes of 256 lanes x 2 rows over the window of `a`
// (AP == 0: the level has none), FP passes over the window of f / row types / code words.
template <int WORDS, int AP, int FP>
struct DuoLoads {
  double tv;
  int32_t to;
  uint64_t rw[WORDS];
  pair_f64x2 a[AP > 0 ? AP : 1];
  pair_f64x2 f[FP];
  double fl[FP];
  uint32_t ty[FP], tl[FP];
  pair_u64x2 c[FP][WORDS], cl[FP];
};
// a_lo / m_lo: the matrix rows of aw[0] / of window index 0 (even, may be negative); AW / W: rows
template <int WORDS, bool TYPES, int AP, int FP>
__device__ __forceinline__ void duo_issue(DuoLoads<WORDS, AP, FP>& g, int n, int a_lo, int AW, int m_lo,
                                          int W, const uint64_t* __restrict__ codes,
                                          const uint8_t* __restrict__ rtype,
                                          const uint64_t* __restrict__ rwords,
                                          const int32_t* __restrict__ doff,
                                          const double* __restrict__ dval, int ntab, const double* a,
                                          const double* __restrict__ f) {
  const int t = threadIdx.x;
  g.tv = t < ntab ? dval[t] : 0.0;
  g.to = t < ntab ? doff[t] : 0;
#pragma unroll
  for (int k = 0; k < WORDS; ++k) g.rw[k] = TYPES ? rwords[t * WORDS + k] : 0;
#pragma unroll
  for (int k = 0; k < AP; ++k) {
    const int idx = (k * 256 + t) * 2;
    const int row = a_lo + idx;  // even: a pair is either entirely before row 0 or not at all
    g.a[k].x = g.a[k].y = 0.0;
    if (idx < AW && row >= 0) {
      if (row + 1 < n) g.a[k] = *reinterpret_cast<const pair_f64x2*>(a + row);
      else if (row < n) g.a[k].x = a[row];
    }
  }
  bool both[FP], lone[FP];
#pragma unroll
  for (int k = 0; k < FP; ++k) {
    const int lw = (k * 256 + t) * 2, row0 = m_lo + lw;
    const bool inside = row0 >= 0 && lw < W;
    both[k] = inside && row0 + 1 < n;
    lone[k] = inside && row0 + 1 == n;
    g.f[k].x = g.f[k].y = g.fl[k] = 0.0;
    if (f) {  // (down-leg, level l+1: f is formed in LDS)
      if (both[k]) g.f[k] = *reinterpret_cast<const pair_f64x2*>(f + row0);
      if (lone[k]) g.fl[k] = f[row0];
    }
  }
#pragma unroll
  for (int k = 0; k < FP; ++k) {
    const int row0 = m_lo + (k * 256 + t) * 2;
    if (TYPES) {
      g.ty[k] = 0xFFFFu;
      g.tl[k] = 0xFFu;
      if (both[k]) g.ty[k] = *reinterpret_cast<const uint16_t*>(rtype + row0);
      if (lone[k]) g.tl[k] = rtype[row0];
    } else {
      g.cl[k].x = g.cl[k].y = ~(uint64_t)0;
#pragma unroll
      for (int j = 0; j < WORDS; ++j) g.c[k][j].x = g.c[k][j].y = ~(uint64_t)0;
      const uint64_t* cp = codes + (int64_t)row0 * WORDS;
      if (both[k]) {
#pragma unroll
        for (int j = 0; j < WORDS; ++j) g.c[k][j] = reinterpret_cast<const pair_u64x2*>(cp)[j];
      }
      if (lone[k]) {
        if (WORDS == 2) g.cl[k] = *reinterpret_cast<const pair_u64x2*>(cp);
        else g.cl[k].x = cp[0];
      }
    }
  }
}
// fw == nullptr: f is not committed (the caller forms it)
template <int WORDS, bool TYPES, int AP, int FP>
__device__ __forceinline__ void duo_commit(const DuoLoads<WORDS, AP, FP>& g, int n, int AW, int m_lo, int W,
                                           uint64_t* wc, uint16_t* tw, double* aw, double* fw) {
  const int t = threadIdx.x;
  if (TYPES) {
#pragma unroll
    for (int k = 0; k < WORDS; ++k) wc[t * WORDS + k] = g.rw[k];
  }
#pragma unroll
  for (int k = 0; k < AP; ++k) {
    const int idx = (k * 256 + t) * 2;
    if (idx < AW) *reinterpret_cast<pair_f64x2*>(aw + idx) = g.a[k];
  }
#pragma unroll
  for (int k = 0; k < FP; ++k) {
    const int lw = (k * 256 + t) * 2;
    if (lw >= W) continue;
    const bool both = m_lo + lw >= 0 && m_lo + lw + 1 < n;  // else: the lone last row, or no row at all
    if (fw) {
      pair_f64x2 fv = g.f[k];
      fv.x = both ? fv.x : g.fl[k];
      *reinterpret_cast<pair_f64x2*>(fw + lw) = fv;
    }
    if (TYPES) {
      uint32_t tl = g.tl[k];
      asm volatile("" : "+v"(tl));  // see dict_pair_commit
      tw[lw >> 1] = (uint16_t)(both ? g.ty[k] : (tl | 0xFF00u));
    } else {
      pair_u64x2* wp = reinterpret_cast<pair_u64x2*>(wc + lw * WORDS);
      wp[0] = both ? g.c[k][0] : g.cl[k];
      if (WORDS == 2) wp[1] = g.c[k][WORDS - 1];
    }
  }
}
// One stage on a window: rows [lo, lo + cnt) (window indices, lo even) of the level whose f / row
// types / code words are fw / tw / wc with W rows from matrix row m_lo; x[xs + i] is the operand of
// window row i.  Results go to out[i - lo] (0.0 for rows outside the matrix) and, for the matrix rows
// in [own_lo, own_hi), to gout if given.
template <int MODE, int WORDS, int UN>
__device__ __forceinline__ void duo_stage(int n, int m_lo, int W, int lo, int cnt, bool types,
                                          const DictEntry* tab, const uint64_t* wc, const uint16_t* tw,
                                          const double* fw, const double* x, int xs, double omega,
                                          double* out, double* gout, int own_lo, int own_hi) {
  for (int base = 0; base < cnt; base += 512) {
    const int k = base + (int)threadIdx.x * 2;
    const bool in = k < cnt;
    const int lw = in ? lo + k : W;  // W: no row
    const int row0 = m_lo + lw;
    DictStream<WORDS, 2> s;
    dict_pair_stream<WORDS>(s, lw, W, row0, n, types, wc, tw, fw);
    if (in && mode_jac(MODE)) {
      s.xi[0] = x[xs + lw];
      s.xi[1] = x[xs + lw + 1];
    }
    if (types) dict_expand<WORDS, 2>(s, wc);
    double res[2];
    dict_rows<MODE, WORDS, UN, 2>(s, in ? xs + lw : 0, tab, x, omega, 0, res);
    if (in) {
      out[k] = s.live[0] ? res[0] : 0.0;
      out[k + 1] = s.live[1] ? res[1] : 0.0;
      if (gout) {
#pragma unroll
        for (int r = 0; r < 2; ++r)
          if (s.live[r] && row0 + r >= own_lo && row0 + r < own_hi) gout[row0 + r] = res[r];
      }
    }
  }
}
// Restriction of the residuals rs (rs[0] = fine row 2 c_lo) to the coarse rows c_lo + q, q < cnt, and
// their first Jacobi sweep from zero: dict_restrict_tail's sums and guards.  fo / vo: LDS windows
// (or null), fH / uH1: global, rows in [own_lo, own_hi) only; d[q]: the coarse diagonal, preloaded.
__device__ __forceinline__ void duo_restrict_row(int c, int n, int nH, const double* rs, int q, double d,
                                                 double omega, double& sum_out, double& v_out) {
  double sum = 0.0, v = 0.0;
  if (c >= 0 && c < nH) {
    const int64_t i = 2 * (int64_t)c;  // linear_restrict_kernel, same guards and order
    if (i < n) sum += 0.5 * rs[2 * q];
    if (i + 1 < n) sum += 1.0 * rs[2 * q + 1];
    if (i + 2 < n) sum += 0.5 * rs[2 * q + 2];
    const double xi = 0.0, acc = 0.0;  // jacobi_from_zero_kernel
    v = (d == 0.0) ? xi : xi + omega * ((sum - acc) / d - xi);
  }
  sum_out = sum;
  v_out = v;
}

template <int W0, int U0, int W1, int U1>
__global__ __launch_bounds__(256) void dict_duo_down_kernel(
    int n0, const uint64_t* __restrict__ codes0, const uint8_t* __restrict__ rtype0,
    const uint64_t* __restrict__ rwords0, const int32_t* __restrict__ doff0,
    const double* __restrict__ dval0, int ntab0, int hbw0,
    int n1, const uint64_t* __restrict__ codes1, const uint8_t* __restrict__ rtype1,
    const uint64_t* __restrict__ rwords1, const int32_t* __restrict__ doff1,
    const double* __restrict__ dval1, int ntab1, int hbw1,
    const double* a0, const double* __restrict__ f0, double* u0_out, double* r0_out,
    double* __restrict__ f1_out, const double* __restrict__ diag1, double* u1_out, double* r1_out,
    int n2, double* __restrict__ f2_out, const double* __restrict__ diag2, double* __restrict__ v2_out,
    double omega, int T, int xcd_map) {
  constexpr int WC0 = DUO_D_M0 * W0, WC1 = (DUO_D_M1 > 256 ? DUO_D_M1 : 256) * W1;
  __shared__ DictEntry tab[256];
  __shared__ __attribute__((aligned(16))) uint64_t wc0[WC0];
  __shared__ __attribute__((aligned(16))) uint64_t wc1[WC1];
  __shared__ uint16_t tw0[DUO_D_M0 / 2];
  __shared__ uint16_t tw1[DUO_D_M1 / 2];
  __shared__ __attribute__((aligned(16))) double aw0[DUO_D_A0];  // tmp_l; then the residuals of l
  __shared__ __attribute__((aligned(16))) double fw0[DUO_D_M0];  // f_l; then f_{l+1} and its first sweep
  __shared__ __attribute__((aligned(16))) double uw0[DUO_D_M0];  // u_l; then u_{l+1} and the residuals of l+1
  static_assert(2 * DUO_D_M1 <= DUO_D_M0 && DUO_D_M1 + DUO_T / 2 + 8 <= DUO_D_M0, "the aliases fit");
  double* rs0 = aw0;
  double* fw1 = fw0;
  double* vw1 = fw0 + DUO_D_M1;
  double* uw1 = uw0;
  double* rs1 = uw0 + DUO_D_M1;
  int w[DW_COUNT];
  duo_windows(hbw0, hbw1, T, w);
  const int tile = xcd_tile(blockIdx.x, gridDim.x, xcd_map);
  const int t0 = tile * T, ce = (t0 / 2) & ~1, b0 = 2 * ce;
  const int m0 = b0 - w[DW_D_M0_LO], M0 = w[DW_D_M0], A0 = w[DW_D_A0];
  const int m1 = ce - w[DW_D_M1_LO], M1 = w[DW_D_M1];
  const bool types0 = rtype0 != nullptr, types1 = rtype1 != nullptr;
  const int t = threadIdx.x;
  DuoLoads<W0, (DUO_D_A0 / 2 + 255) / 256, DUO_D_M0 / 512> g0;
  DuoLoads<W1, 0, 1> g1;
  if (types0) duo_issue<W0, true>(g0, n0, m0 - hbw0, A0, m0, M0, codes0, rtype0, rwords0, doff0, dval0, ntab0, a0, f0);
  else duo_issue<W0, false>(g0, n0, m0 - hbw0, A0, m0, M0, codes0, rtype0, rwords0, doff0, dval0, ntab0, a0, f0);
  if (types1) duo_issue<W1, true>(g1, n1, 0, 0, m1, M1, codes1, rtype1, rwords1, doff1, dval1, ntab1, nullptr, nullptr);
  else duo_issue<W1, false>(g1, n1, 0, 0, m1, M1, codes1, rtype1, rwords1, doff1, dval1, ntab1, nullptr, nullptr);
  // the coarse diagonals: rows m1 + 2 t, + 1 of level l+1; the owned row cc_lo + t of level l+2
  pair_f64x2 d1;
  d1.x = d1.y = 0.0;
  {
    const int c = m1 + 2 * t;
    if (2 * t < M1 && c >= 0) {
      if (c + 1 < n1) d1 = *reinterpret_cast<const pair_f64x2*>(diag1 + c);
      else if (c < n1) d1.x = diag1[c];
    }
  }
  int own[6];
  duo_owned(t0, T, own);
  const int cc_lo = own[4], cc_hi = min(own[5], n2);
  const double d2 = cc_lo + t < cc_hi ? diag2[cc_lo + t] : 0.0;
  dict_put_table<CSR_JACOBI>(tab, g0.tv, g0.to, ntab0);
  if (types0) duo_commit<W0, true>(g0, n0, A0, m0, M0, wc0, tw0, aw0, fw0);
  else duo_commit<W0, false>(g0, n0, A0, m0, M0, wc0, tw0, aw0, fw0);
  if (types1) duo_commit<W1, true>(g1, n1, 0, m1, M1, wc1, tw1, nullptr, nullptr);
  else duo_commit<W1, false>(g1, n1, 0, m1, M1, wc1, tw1, nullptr, nullptr);
  __syncthreads();
  // level l: second pre-sweep (tmp_l -> u_l), residual
  duo_stage<CSR_JACOBI, W0, U0>(n0, m0, M0, 0, M0, types0, tab, wc0, tw0, fw0, aw0, hbw0, omega, uw0, u0_out,
                                own[0], own[1]);
  __syncthreads();
  dict_put_table<CSR_RESID>(tab, g0.tv, g0.to, ntab0);
  __syncthreads();
  duo_stage<CSR_RESID, W0, U0>(n0, m0, M0, hbw0, w[DW_D_R0], types0, tab, wc0, tw0, fw0, uw0, 0, omega, rs0,
                               r0_out, own[0], own[1]);
  __syncthreads();
  // restriction to the window of level l+1 and its first sweep from zero (kept in LDS)
  const int c_own = own[2], c_end = own[3];
  if (2 * t < M1) {
    double fv[2], vv[2];
    duo_restrict_row(m1 + 2 * t, n0, n1, rs0, 2 * t, d1.x, omega, fv[0], vv[0]);
    duo_restrict_row(m1 + 2 * t + 1, n0, n1, rs0, 2 * t + 1, d1.y, omega, fv[1], vv[1]);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int c = m1 + 2 * t + r;
      fw1[2 * t + r] = fv[r];
      vw1[2 * t + r] = vv[r];
      if (c >= c_own && c < c_end && c < n1) f1_out[c] = fv[r];
    }
  }
  dict_put_table<CSR_JACOBI>(tab, g1.tv, g1.to, ntab1);
  __syncthreads();
  // level l+1: second pre-sweep, residual
  duo_stage<CSR_JACOBI, W1, U1>(n1, m1, M1, hbw1, w[DW_D_U1], types1, tab, wc1, tw1, fw1, vw1, 0, omega, uw1,
                                u1_out, c_own, c_end);
  __syncthreads();
  dict_put_table<CSR_RESID>(tab, g1.tv, g1.to, ntab1);
  __syncthreads();
  duo_stage<CSR_RESID, W1, U1>(n1, m1, M1, 2 * hbw1, w[DW_D_R1], types1, tab, wc1, tw1, fw1, uw1, -hbw1, omega,
                               rs1, r1_out, c_own, c_end);
  __syncthreads();
  // restriction to the owned rows of level l+2 and their first sweep
  if (cc_lo + t < cc_hi) {
    const int cc = cc_lo + t;
    double fv, vv;
    // rs1[0] is row ce of level l+1; row 2 cc sits at 2 cc - ce
    duo_restrict_row(cc, n1, n2, rs1 + (2 * cc - ce) - 2 * t, t, d2, omega, fv, vv);
    f2_out[cc] = fv;
    v2_out[cc] = vv;
  }
}
template <int W0, int U0, int W1, int U1>
__global__ __launch_bounds__(256) void dict_duo_up_kernel(
    int n0, const uint64_t* __restrict__ codes0, const uint8_t* __restrict__ rtype0,
    const uint64_t* __restrict__ rwords0, const int32_t* __restrict__ doff0,
    const double* __restrict__ dval0, int ntab0, int hbw0,
    int n1, const uint64_t* __restrict__ codes1, const uint8_t* __restrict__ rtype1,
    const uint64_t* __restrict__ rwords1, const int32_t* __restrict__ doff1,
    const double* __restrict__ dval1, int ntab1, int hbw1,
    const double* a1, const double* __restrict__ f1, double* u1_out,
    const double* u0_in, const double* __restrict__ f0, double* u0_out,
    double omega, int n_h, const double* uh_in, double* uh_out, int T, int xcd_map) {
  constexpr int WC0 = DUO_U_M0 * W0, WC1 = DUO_U_M1 * W1;
  __shared__ DictEntry tab[256];
  __shared__ __attribute__((aligned(16))) uint64_t wc0[WC0];
  __shared__ __attribute__((aligned(16))) uint64_t wc1[WC1];
  __shared__ uint16_t tw0[DUO_U_M0 / 2];
  __shared__ uint16_t tw1[DUO_U_M1 / 2];
  __shared__ __attribute__((aligned(16))) double aw1[DUO_U_A1];  // tmp_{l+1}; then u_{l+1}
  __shared__ __attribute__((aligned(16))) double fw1[DUO_U_M1];
  __shared__ __attribute__((aligned(16))) double uw1[DUO_U_M1];
  __shared__ __attribute__((aligned(16))) double aw0[DUO_U_A0];  // u_l, + P u_{l+1}; then the frame of u_l
  __shared__ __attribute__((aligned(16))) double fw0[DUO_U_M0];
  __shared__ __attribute__((aligned(16))) double uw0[DUO_U_M0];
  double* vw1 = aw1;
  double* rs = aw0;
  int w[DW_COUNT];
  duo_windows(hbw0, hbw1, T, w);
  const int tile = xcd_tile(blockIdx.x, gridDim.x, xcd_map);
  const int t0 = tile * T, ce = (t0 / 2) & ~1;
  const int m0 = t0 - hbw0, M0 = w[DW_U_M0], A0 = w[DW_U_A0];
  const int m1 = ce - w[DW_U_M1_LO], M1 = w[DW_U_M1], A1 = w[DW_U_A1];
  const bool types0 = rtype0 != nullptr, types1 = rtype1 != nullptr;
  const int t = threadIdx.x;
  DuoLoads<W1, (DUO_U_A1 / 2 + 255) / 256, 1> g1;
  DuoLoads<W0, (DUO_U_A0 / 2 + 255) / 256, (DUO_U_M0 + 511) / 512> g0;
  if (types1) duo_issue<W1, true>(g1, n1, m1 - hbw1, A1, m1, M1, codes1, rtype1, rwords1, doff1, dval1, ntab1, a1, f1);
  else duo_issue<W1, false>(g1, n1, m1 - hbw1, A1, m1, M1, codes1, rtype1, rwords1, doff1, dval1, ntab1, a1, f1);
  if (types0) duo_issue<W0, true>(g0, n0, m0 - hbw0, A0, m0, M0, codes0, rtype0, rwords0, doff0, dval0, ntab0, u0_in, f0);
  else duo_issue<W0, false>(g0, n0, m0 - hbw0, A0, m0, M0, codes0, rtype0, rwords0, doff0, dval0, ntab0, u0_in, f0);
  pair_f64x2 pre[2];  // uh_in may be uh_out: a lane reads only the rows it later writes
  double pre1;
  if (T == DUO_T) dict_prolong_pre<DUO_T>(tile, n0, n_h, uh_in, pre, pre1);  // (T is one of the two)
  else dict_prolong_pre<DUO_T_SMALL>(tile, n0, n_h, uh_in, pre, pre1);
  dict_put_table<CSR_JACOBI>(tab, g1.tv, g1.to, ntab1);
  if (types1) duo_commit<W1, true>(g1, n1, A1, m1, M1, wc1, tw1, aw1, fw1);
  else duo_commit<W1, false>(g1, n1, A1, m1, M1, wc1, tw1, aw1, fw1);
  if (types0) duo_commit<W0, true>(g0, n0, A0, m0, M0, wc0, tw0, aw0, fw0);
  else duo_commit<W0, false>(g0, n0, A0, m0, M0, wc0, tw0, aw0, fw0);
  __syncthreads();
  // level l+1: both post-sweeps
  duo_stage<CSR_JACOBI, W1, U1>(n1, m1, M1, 0, M1, types1, tab, wc1, tw1, fw1, aw1, hbw1, omega, uw1, nullptr, 0, 0);
  __syncthreads();
  int own[6];
  duo_owned(t0, T, own);
  const int c_own = own[2], c_end = own[3];
  duo_stage<CSR_JACOBI, W1, U1>(n1, m1, M1, hbw1, w[DW_U_S1], types1, tab, wc1, tw1, fw1, uw1, 0, omega, vw1,
                                u1_out, c_own, c_end);
  __syncthreads();
  dict_put_table<CSR_JACOBI>(tab, g0.tv, g0.to, ntab0);
  // u_l + P u_{l+1} on the window of level l: linear_prolong_add2_kernel per coarse point j, fine rows
  // 2j, 2j + 1.  vw1[0] is row s1 = ce - (hbw0 + 2) of level l+1, aw0[0] row m0 - hbw0 of level l.
  {
    const int s1 = ce - w[DW_U_S1_LO], a_lo = m0 - hbw0;
    for (int k = 2 * t; k < A0; k += 512) {
      const int i = a_lo + k;  // even
      if (i < 0 || i >= n0) continue;
      const int j = i >> 1;
      double p0 = 0.0, p1 = 0.0;
      const double b = (j < n1) ? vw1[j - s1] : 0.0;
      if (j >= 1 && j - 1 < n1) p0 += 0.5 * vw1[j - 1 - s1];
      if (j < n1) {
        p0 += 0.5 * b;
        p1 += 1.0 * b;
      }
      aw0[k] = aw0[k] + p0;
      if (i + 1 < n0) aw0[k + 1] = aw0[k + 1] + p1;
    }
  }
  __syncthreads();
  // level l: both post-sweeps; the second one rests in tmp_l (u0_out) and feeds the prolongation
  duo_stage<CSR_JACOBI, W0, U0>(n0, m0, M0, 0, M0, types0, tab, wc0, tw0, fw0, aw0, hbw0, omega, uw0, nullptr, 0, 0);
  __syncthreads();
  duo_stage<CSR_JACOBI, W0, U0>(n0, m0, M0, hbw0, w[DW_U_S0], types0, tab, wc0, tw0, fw0, uw0, 0, omega, rs, u0_out,
                                own[0], own[1]);
  __syncthreads();
  if (T == DUO_T) dict_prolong_tail<DUO_T>(tile, n0, rs, n_h, pre, pre1, uh_out);
  else dict_prolong_tail<DUO_T_SMALL>(tile, n0, rs, n_h, pre, pre1, uh_out);
}

// ---- K-Patch: the level's whole down-leg / up-leg in ONE pass over the level ------------
// On the big levels (0 and 1 of the 4096^2 hierarchy) every sweep streams f, x and the
// output again, 25 B per row and sweep.  The 2+2 true-Jacobi cycle touches such a level
// five times on the way down (sweep, sweep, residual + restriction) and three times on the
// way up (prolongation, sweep, sweep).  These kernels do each leg in one launch (temporal
// blocking): a workgroup owns a 2-D PATCH of the level -- patch_th(RINGS) grid lines x PATCH_TW
// columns of the flat index (row = line * m + column; m = the pitch of the band: 4096,
// 2048, ...) -- loads it once with the halo the later stages need (one ring of lines and
// columns per stage), and runs the stages LDS -> LDS with a barrier in between.  The halo
// cells are recomputed by the neighbouring patches (same expressions, same bits):
//   down: [sweep 1] -> sweep 2 (stored) -> residual -> restriction + first coarse sweep
//   up:   u + P u_H (formed while loading) -> sweep 1 -> sweep 2 (stored)
// All addressing is flat-index arithmetic: cell (line lj, column li) of a patch is row
// (j0 + lj) m + i0 + li even when i0 + li runs past the end of a grid line (the flat-index
// smear of the reference's coarsening), so a column offset o = dj m + di of the
// pair table is the LDS offset dj * pitch + di.  Row arithmetic = dict_rows' (entries in
// ascending column order, diagonal split off for Jacobi, IEEE divide), transfers =
// dict_restrict_tail / linear_prolong_add2_kernel: the V-cycle stays bit-identical.
// The row's structure comes from its TYPE alone: the host expands type -> code word ->
// pairs into one table of (value, diagonal value, LDS offset) per type and slot, so a
// cell costs one byte of matrix and no decode chain.  Interior rows share one type: the
// table reads of a wave are broadcasts.
constexpr int PATCH_TW = 64;                 // columns of a patch (output)
constexpr int PATCH_EH = 48;                 // lines held: the output lines + RINGS halo lines above and below
// lines of a patch (output).  RINGS = dependent stencil stages a launch runs on the loaded data, one
// ring of halo lines each: 3 for the level-0 down-leg (sweep, sweep, residual) and the colour
// launches -> 42 lines; 2 for every up-leg (sweep, sweep) and the down-legs of the levels >= 1
// (sweep, residual) -> 44 lines in the same held frame, threads and LDS
constexpr int patch_th(int rings) { return PATCH_EH - 2 * rings; }
static bool patch_rings_ok(int rings) { return rings == 2 || rings == 3; }
constexpr int PATCH_EC = PATCH_TW + 8;       // columns held: [-4, TW + 4)
constexpr int PATCH_NT = 432;                // threads = 6 line groups x 72 columns (4 workgroups per CU)
constexpr int PATCH_K = PATCH_EH * PATCH_EC / PATCH_NT;  // cells per thread: 8 consecutive lines
constexpr int PATCH_BUF = (PATCH_EH + 2) * PATCH_EC;     // + one guard line above and below
constexpr int PATCH_MAXTAB = 192;            // table capacity: (types + 1) x slots
// values of a tile flag that are no row type: a column-typed tile / a general one (patch_tile_flags_kernel)
constexpr uint32_t PATCH_FLAG_COLTYPED = 254u, PATCH_FLAG_GENERAL = 255u;
constexpr int PATCH_SEAM_RINGS_HOST = 5;  // (= PATCH_SEAM_RINGS, defined with the seam kernel below)
static_assert(PATCH_EH * PATCH_EC == PATCH_K * PATCH_NT && PATCH_NT % PATCH_EC == 0, "patch geometry");
// The held frame as a parameter of the patch functions: EH lines x EC columns [-CL, EC - CL) around
// the PATCH_TW output columns, PATCH_K consecutive lines per thread.  PatchFrame is the frame of the
// legs above (every function defaults to it); the seam kernel, five dependent stages, holds a
// wider one (patch_seam_kernel).
template <int EH_, int EC_>
struct PatchFrameT {
  static constexpr int EH = EH_, EC = EC_, CL = (EC_ - PATCH_TW) / 2;
  static constexpr int NT = EH_ / PATCH_K * EC_, BUF = (EH_ + 2) * EC_;
  static constexpr int th(int rings) { return EH_ - 2 * rings; }
  static_assert(EH_ % PATCH_K == 0 && (EC_ - PATCH_TW) % 2 == 0 && NT >= PATCH_MAXTAB && NT <= 1024, "patch frame");
};
using PatchFrame = PatchFrameT<PATCH_EH, PATCH_EC>;
static_assert(PatchFrame::NT == PATCH_NT && PatchFrame::BUF == PATCH_BUF && PatchFrame::CL == 4, "patch geometry");

struct PatchJ { double a, d; };              // off-diagonal value (else +0.0), diagonal value (else +0.0)
struct PatchR { double a; int32_t loff, ok; };  // value, LDS offset, slot in use

// The PATCH_K cells one thread owns: column li of the consecutive lines lj0 .. lj0 + 7; cell k
// sits at LDS index cell0 + k * PATCH_EC and is flat row row0 + k m.  Adjacent lanes own
// adjacent columns (conflict-free 8-byte LDS accesses, coalesced global ones), and a thread's
// cells are vertical neighbours, so the wave-uniform path walks them with a sliding 3 x 3
// register window: 3 LDS reads per cell instead of one per matrix entry.
struct PatchCells {
  int cell0, row0, lj0, li;
  double f[PATCH_K];
  uint32_t ty[PATCH_K / 4]; // row types, a byte each, clamped to the all-absent table row `ntypes`
  bool live[PATCH_K];       // row inside the matrix
  bool uniform;             // every cell of the wave has the type tu (then the table comes
  uint32_t tu;              // through scalar loads instead of per-lane LDS reads)
  bool flagged;             // the tile's flag says so for the whole workgroup: ty[] is not filled in
  bool coltyped;            // column-typed tile (flag 254): all PATCH_K cells of the thread have ONE type, the
                            // lane's, kept in ty[0]; every row is inside the matrix
  __device__ __forceinline__ uint32_t type(int k) const {
    return flagged ? tu : (coltyped ? ty[0] : (ty[k >> 2] >> (8 * (k & 3))) & 255u);
  }
  __device__ __forceinline__ uint32_t lane_type() const { return ty[0]; }
};

// The table of ONE row type held in scalar registers (the wave-uniform fast path: in the
// interior of a level every row has the same type).  Loaded once per workgroup through
// scalar loads from the per-type arrays the host lays out (solver.cpp: build_patch_table):
//   utabd: per type aj[UN] (off-diagonal values, +0.0 elsewhere), ar[UN] (values), diag
//   utabi: per type lo[UN] (LDS offsets), jmask (slots with an off-diagonal entry), rmask
//          (slots in use)
// slot s = (dj + 1) * 3 + (di + 1) of the 3 x 3 neighbourhood = ascending column offset
// (-m-1, -m, -m+1, -1, 0, +1, m-1, m, m+1): walking the slots in order IS the reference's
// ascending-column summation order (smoother.hpp:101-117).
//   utabd: per type wj[9] (off-diagonal values, +0.0 where there is no entry and on the
//          diagonal), wr[9] (values, +0.0 where there is no entry), diag
//   utabi: per type rmask (slots in use), corners (1 when a corner slot 0, 2, 6, 8 is in use)
struct PatchU {
  double wj[9], wr[9], diag;
#ifdef AMG_PATCH_FASTDIV
  double rdiag;
#endif
  uint32_t rmask, corners;
};
__device__ __forceinline__ void patch_load_u(PatchU& U, uint32_t tu, const double* __restrict__ utabd,
                                             const int32_t* __restrict__ utabi) {
  const double* d = utabd + (size_t)tu * 19;
  const int32_t* i = utabi + (size_t)tu * 2;
#pragma unroll
  for (int e = 0; e < 9; ++e) {
    U.wj[e] = d[e];
    U.wr[e] = d[9 + e];
  }
  U.diag = d[18];
#ifdef AMG_PATCH_FASTDIV
  U.rdiag = 1.0 / (U.diag == 0.0 ? 1.0 : U.diag);
#endif
  U.rmask = (uint32_t)i[0];
  U.corners = (uint32_t)i[1];
}
// Uniform-type evaluation of the thread's PATCH_K vertically consecutive cells with a sliding
// window: w[r][c] = value of line (k - 1 + r), column (li - 1 + c).  Slots that hold no entry
// have weight +0.0: adding (+0.0) x leaves a Jacobi accumulator's bits alone for finite x (see
// dict_rows); the residual selects them away.  CORNERS = false: the four corner slots are
// not even read (5-point level).
// MASK >= 0: the type's slots in use are exactly MASK (the interior row types of a Poisson
// hierarchy: 0x0BA = 5-point level 0, 0x1D7 = level 1 with its exact-zero +-1 entries pruned,
// 0x1FF = 9-point levels): absent slots are not even multiplied, and the residual needs no
// selects.  Same bits as the generic form (MASK < 0): a Jacobi accumulator starts at +0.0 and
// never becomes -0.0, so skipping a (+0.0) x term changes nothing for finite x; the residual's
// generic form selects absent terms away, which is what not computing them does.
template <bool RESID, bool CORNERS, bool GS = false, int MASK = -1, class FR = PatchFrame>
__device__ __forceinline__ void patch_eval_u(const double* buf, int cell0, const PatchU& U,
                                             const double (&f)[PATCH_K], double omega,
                                             double (&res)[PATCH_K]) {
  const double* p = buf + cell0 - FR::EC;  // line above the first cell
  if (!CORNERS && !RESID && U.diag == 0.0) {  // rows without a diagonal keep their value (smoother.hpp:133)
#pragma unroll
    for (int k = 0; k < PATCH_K; ++k) res[k] = p[(k + 1) * FR::EC];
    return;
  }
  // (5-point rows: the test above is wave-uniform and sits OUTSIDE the cell loop; inside it, it
  // cuts the loop into one basic block per cell and the eight independent dependency chains --
  // LDS read, sums, IEEE division -- run one after the other instead of interleaved.  For the
  // 9-point rows that is what the 72-register budget of four workgroups per CU wants: there the
  // test stays inside the loop, measured 10 % faster on levels 1-3.)
  double w[3][3];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) w[r][c] = (CORNERS || c == 1 || r == 1) ? p[r * FR::EC + c - 1] : 0.0;
#pragma unroll
  for (int k = 0; k < PATCH_K; ++k) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
      w[2][c] = (CORNERS || c == 1) ? p[(k + 2) * FR::EC + c - 1] : 0.0;
    if (!CORNERS) {  // left / right of line k + 1 become the middle row's of the next cell
      w[2][0] = p[(k + 2) * FR::EC - 1];
      w[2][2] = p[(k + 2) * FR::EC + 1];
    }
    const double xi = w[1][1];
    if (RESID) {
      double acc = f[k];
#pragma unroll
      for (int s9 = 0; s9 < 9; ++s9) {
        const int r = s9 / 3, c = s9 % 3;
        if (!CORNERS && r != 1 && c != 1) continue;
        if (MASK >= 0) {
          if ((MASK >> s9) & 1) acc -= U.wr[s9] * w[r][c];
        } else {
          double t = U.wr[s9] * w[r][c];
          t = ((U.rmask >> s9) & 1u) ? t : 0.0;
          acc -= t;
        }
      }
      res[k] = acc;
    } else {
      double acc = 0.0;
#pragma unroll
      for (int s9 = 0; s9 < 9; ++s9) {
        const int r = s9 / 3, c = s9 % 3;
        if (s9 == 4 || (!CORNERS && r != 1 && c != 1)) continue;
        if (MASK >= 0 && !((MASK >> s9) & 1)) continue;
        acc += U.wj[s9] * w[r][c];
      }
      if (CORNERS && U.diag == 0.0) {
        res[k] = xi;
      } else {
#ifdef AMG_PATCH_FASTDIV
        // experiment: Markstein's correctly rounded quotient from the (wave-uniform) reciprocal
        const double nm = f[k] - acc;
        const double q0 = nm * U.rdiag;
        const double r0 = __builtin_fma(-U.diag, q0, nm);
        const double q1 = __builtin_fma(r0, U.rdiag, q0);
        const double r1 = __builtin_fma(-U.diag, q1, nm);
        const double q = __builtin_fma(r1, U.rdiag, q1);
#else
        const double q = (f[k] - acc) / U.diag;  // smoother.hpp:136
#endif
        res[k] = GS ? q : xi + omega * (q - xi);      // GS: the Gauss-Seidel update itself (K-SELL CSR_GS)
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      w[0][c] = w[1][c];
      w[1][c] = w[2][c];
    }
  }
}
// Column-typed tiles (flag 254: the tiles at the line ends): the lane-typed twin of patch_eval_u.  All
// PATCH_K cells of a thread share the lane's row type, so the thread walks them with the same sliding
// 3 x 3 window -- 3 LDS reads per cell at static addresses instead of one dependent read per entry --
// and takes its weights from the slot-form table of ITS type, which the workgroup staged in LDS in the
// place of the per-entry tables (patch_load):
//   ctabJ: per type wj[9] (off-diagonal values; +0.0 on the diagonal and where there is no entry), diag
//   ctabR: per type wr[9] (values; +0.0 where there is no entry), rmask (the slots in use, as an integer)
// The weights are re-read for every cell, half a row at a time (9 + 3 reads per cell; patch_eval: 28,
// with addresses that hang on a loaded offset): beside the window's 18 registers, f and the results, a
// lane's 9 weights held for the stage do not fit the 72 registers of four workgroups per CU.
// BAR: scheduling barriers keep the compiler from issuing the reads of several cells at once, which
// costs the same registers: the up-legs (72 registers) spill 3 registers without them and none with
// them; the 7- and 9-point down-legs and the seam (80) spill none without them and 5-7 with them.  The
// 5-point down-leg (72) spills either way and keeps the general path (profiles/coltype_isa.md).
// Same bits as patch_eval: the slots in ascending order ARE the entries in ascending column order; an
// absent slot adds (+0.0) x to a Jacobi accumulator that starts at +0.0 (the argument of patch_eval_u's
// generic form) and is selected away in the residual; diag is the same sum of the type's entries; a lane
// without a diagonal keeps its value and divides by 1.0.
constexpr int PATCH_CT = 10;  // doubles per type in ctabJ / ctabR
static_assert((PATCH_MAXTAB / 5) * PATCH_CT * sizeof(double) <= PATCH_MAXTAB * 16,
              "the slot tables of (ntypes + 1) <= PATCH_MAXTAB / 5 types fit tabJ and tabR");
template <bool RESID, bool BAR, class FR = PatchFrame>
__device__ __forceinline__ void patch_eval_c(const double* buf, int cell0, uint32_t tl, const double* ctab,
                                             const double (&f)[PATCH_K], double omega, double (&res)[PATCH_K]) {
  const double* p = buf + cell0 - FR::EC;  // line above the first cell
  int to = (int)tl * PATCH_CT;
  uint32_t rmask = 0;
  if (RESID) rmask = reinterpret_cast<const uint32_t*>(ctab + to + 9)[0];
  double w[3][3];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) w[r][c] = p[r * FR::EC + c - 1];
#pragma unroll
  for (int k = 0; k < PATCH_K; ++k) {
    // (!BAR: the table offset is opaque per cell, else the compiler hoists the weights of all cells into
    // registers: the seam kernel then spills 8 of them)
    if (!BAR) asm("" : "+v"(to));
    const double* wt = ctab + to;
#pragma unroll
    for (int c = 0; c < 3; ++c) w[2][c] = p[(k + 2) * FR::EC + c - 1];
    const double xi = w[1][1];
    double acc = RESID ? f[k] : 0.0;
#pragma unroll
    for (int s9 = 0; s9 < 9; ++s9) {
      if (BAR && s9 == 5) __builtin_amdgcn_sched_barrier(0);  // the second half of the weights after the first is used up
      if (!RESID && s9 == 4) continue;
      const double t = wt[s9] * w[s9 / 3][s9 % 3];
      if (RESID) acc -= ((rmask >> s9) & 1u) ? t : 0.0;
      else acc += t;
    }
    if (RESID) {
      res[k] = acc;
    } else {
      const double diag = wt[9];
      const bool nod = diag == 0.0;
      const double q = (f[k] - acc) / (nod ? 1.0 : diag);  // smoother.hpp:136
      res[k] = nod ? xi : xi + omega * (q - xi);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      w[0][c] = w[1][c];
      w[1][c] = w[2][c];
    }
    if (BAR) __builtin_amdgcn_sched_barrier(0);  // one cell's reads at a time
  }
}
// Row arithmetic of dict_rows, per-lane table entries from the LDS copy (mixed row types:
// level boundaries).
template <int UN, bool RESID, bool GS = false>
__device__ __forceinline__ double patch_eval(const double* buf, int cell, uint32_t type,
                                             const PatchJ* tabJ, const PatchR* tabR, double fi,
                                             double omega) {
  const int t0 = (int)type * UN;
  double xx[UN];
  if (RESID) {
    double av[UN];
    bool ok[UN];
#pragma unroll
    for (int e = 0; e < UN; ++e) {
      const PatchR r = tabR[t0 + e];
      av[e] = r.a;
      ok[e] = r.ok != 0;
      xx[e] = buf[cell + r.loff];
    }
    double acc = fi;
#pragma unroll
    for (int e = 0; e < UN; ++e) {
      double t = av[e] * xx[e];
      t = ok[e] ? t : 0.0;
      acc -= t;
    }
    return acc;
  }
  double aj[UN], dj[UN];
#pragma unroll
  for (int e = 0; e < UN; ++e) {
    const PatchJ j = tabJ[t0 + e];
    aj[e] = j.a; dj[e] = j.d;
    xx[e] = buf[cell + tabR[t0 + e].loff];
  }
  double acc = 0.0, diag = 0.0;
  const double xi = buf[cell];
#pragma unroll
  for (int e = 0; e < UN; ++e) {
    acc += aj[e] * xx[e];
    diag += dj[e];
  }
  const bool nod = diag == 0.0;
  const double q = (fi - acc) / (nod ? 1.0 : diag);  // smoother.hpp:136
  return nod ? xi : (GS ? q : xi + omega * (q - xi));
}

// one stage over the region lines [l0, l1) x columns [c0, c1), IN PLACE in the workgroup's one
// LDS buffer: every thread evaluates its PATCH_K cells into registers (branch-free, so the
// LDS reads overlap), the workgroup meets at a barrier, then the results are written back
// (one buffer instead of two: four workgroups of 432 threads fit a CU instead of one, which is what these
// latency-bound stages need).  Cells outside the region or outside the matrix keep their
// value; ZERO: such cells inside the region are set to 0.0 instead (the residual that the
// restriction reads).  out (optional): rows of the patch proper also go to global memory.
template <int UN, int UM, bool RESID, bool NT, bool ZERO, int TH, class FR = PatchFrame, bool CBAR = false>
__device__ __forceinline__ void patch_stage(const PatchCells& pc, int m, int ntypes, double* buf,
                                            const PatchU& U, const PatchJ* tabJ, const PatchR* tabR,
                                            double omega, int l0, int l1, int c0, int c1, double* out) {
  const bool inc = pc.li >= c0 && pc.li < c1;
  double res[PATCH_K];
  bool did[PATCH_K], inr[PATCH_K];
#pragma unroll
  for (int k = 0; k < PATCH_K; ++k) {
    const int lj = pc.lj0 + k;
    inr[k] = inc && lj >= l0 && lj < l1;
    did[k] = inr[k] && pc.live[k];
  }
  if (pc.uniform && U.rmask == (uint32_t)UM) {
    // interior of the level (UM = the slots its row type uses, chosen at launch): one row type
    // for the whole wave, weights in scalar registers; cells outside the region are evaluated
    // with it too (their reads stay inside the guard lines) and dropped.  Every other wave
    // (level boundaries) takes the per-lane table.
    patch_eval_u<RESID, (UM & 0x145) != 0, false, (UM & 0x145) ? -1 : UM, FR>(buf, pc.cell0, U, pc.f, omega, res);
  } else if (pc.coltyped) {
    // a tile at a line end: the lane's type for all its cells (every row is inside the matrix; cells
    // outside the region are evaluated and dropped, as on the scalar path)
    patch_eval_c<RESID, CBAR, FR>(buf, pc.cell0, pc.lane_type(),
                            reinterpret_cast<const double*>(RESID ? (const void*)tabR : (const void*)tabJ), pc.f, omega, res);
  } else {
#pragma unroll
    for (int k = 0; k < PATCH_K; ++k)
      res[k] = patch_eval<UN, RESID>(buf, pc.cell0 + k * FR::EC,
                                     did[k] ? pc.type(k) : (uint32_t)ntypes, tabJ, tabR, pc.f[k], omega);
  }
  lds_barrier();  // everybody has read the old values
  const bool outc = out != nullptr && pc.li >= 0 && pc.li < PATCH_TW;
#pragma unroll
  for (int k = 0; k < PATCH_K; ++k) {
    if (did[k]) buf[pc.cell0 + k * FR::EC] = res[k];
    else if (ZERO && inr[k]) buf[pc.cell0 + k * FR::EC] = 0.0;
    const int lj = pc.lj0 + k;
    if (outc && did[k] && lj >= 0 && lj < TH) {
      double* op = out + (pc.row0 + k * m);
      if (NT) __builtin_nontemporal_store(res[k], op);
      else *op = res[k];
    }
  }
}

// The smoothed patch leaves through LDS: 64 consecutive threads write one 512-byte line of the
// patch, so every store of a wave covers whole, aligned 128-byte lines.  (Stored straight from
// the stage's registers, a line was split 60 + 4 entries between two waves -- the thread map
// has 72 columns -- and the PMC write traffic was 1.5 x the vector.)
template <bool NT, int RINGS, class FR = PatchFrame>
__device__ __forceinline__ void patch_copy_out(const double* buf, double* __restrict__ out, int n, int m,
                                               int j0, int i0) {
  for (int q = threadIdx.x; q < FR::th(RINGS) * PATCH_TW; q += FR::NT) {
    const int lj = q / PATCH_TW, li = q - lj * PATCH_TW;
    const int64_t row = (int64_t)(j0 + lj) * m + i0 + li;
    if (row < (int64_t)n) {
      const double v = buf[(lj + RINGS + 1) * FR::EC + li + FR::CL];
      if (NT) __builtin_nontemporal_store(v, out + row);
      else out[row] = v;
    }
  }
}

struct __attribute__((aligned(8))) PatchPair { double x, y; };  // 16-byte load, 8-byte aligned

// flag[idx] of a per-tile flag array, for a workgroup-uniform idx: the aligned 32-bit word that holds
// the byte comes through a scalar load, so nothing on the vector side waits for it (the arrays are
// padded to whole words where they are allocated: solver.cpp)
__device__ __forceinline__ uint32_t patch_flag(const uint8_t* __restrict__ flag, int idx) {
  const uint32_t* __restrict__ w = reinterpret_cast<const uint32_t*>(flag);
  return (w[idx >> 2] >> (8 * (idx & 3))) & 255u;
}

// The per-lane tables in LDS (patch_eval): thread t loads row t of ptab (nent x {aJ, d, aR, loff as
// double; -1e9 = unused slot}) into registers (patch_issue_tables) and writes it later, behind
// loads issued after it (patch_stage_tables); slots past nent: absent.  One row per thread covers
// the table.
static_assert(PATCH_MAXTAB <= PATCH_NT, "one table row per thread");
struct PatchTabRow { double v[4]; };
__device__ __forceinline__ void patch_issue_tables(PatchTabRow& tb, const double* __restrict__ ptab, int nent) {
  const int t = (int)threadIdx.x < nent ? (int)threadIdx.x : 0;  // (nent >= 1: threads past it re-read row 0)
#pragma unroll
  for (int q = 0; q < 4; ++q) tb.v[q] = ptab[4 * t + q];
}
template <class FR = PatchFrame>
__device__ __forceinline__ void patch_stage_tables(PatchJ* tabJ, PatchR* tabR, const PatchTabRow& tb, int nent) {
  const int t = threadIdx.x;
  if (t >= PATCH_MAXTAB) return;
  PatchJ j = {0.0, 0.0};
  PatchR r = {0.0, 0, 0};
  if (t < nent) {
    j.a = tb.v[0];
    j.d = tb.v[1];
    r.a = tb.v[2];
    const double lo = tb.v[3];
    r.ok = lo > -1.0e8 ? 1 : 0;
    r.loff = r.ok ? (int)lo : 0;
    // the table's offsets dj * PATCH_EC + di (|di| <= 1) in a frame of another pitch
    if (FR::EC != PATCH_EC) r.loff += (r.loff > PATCH_EC / 2 ? 1 : (r.loff < -PATCH_EC / 2 ? -1 : 0)) * (FR::EC - PATCH_EC);
  }
  tabJ[t] = j;
  tabR[t] = r;
}
// guard lines: finite values for the reads of dropped cells
template <class FR = PatchFrame>
__device__ __forceinline__ void patch_clear_guards(double* buf) {
  for (int t = threadIdx.x; t < 2 * FR::EC; t += FR::NT)
    buf[t < FR::EC ? t : FR::BUF - 2 * FR::EC + t] = 0.0;
}
// The rest of the common prologue, after the cells (patch_load): guards, and the per-lane tables
// where a flagged tile needs them.  Only a wave that is not on the scalar path reads them
// (patch_stage: pc.uniform && U.rmask == UM).  On a flagged tile every wave has the type pc.tu, so
// the tables are read only when that type is not the kernel kind's (a rare tile: a dependent load
// here); every other flagged tile neither loads nor writes them.  A tile without a flag staged
// them in patch_load, beside its row types.
template <int UM, class FR = PatchFrame>
__device__ __forceinline__ void patch_prologue(const PatchCells& pc, const PatchU& U, double* buf, PatchJ* tabJ,
                                               PatchR* tabR, const double* __restrict__ ptab, int nent) {
  if (pc.flagged && U.rmask != (uint32_t)UM) {
    PatchTabRow tb;
    patch_issue_tables(tb, ptab, nent);
    patch_stage_tables<FR>(tabJ, tabR, tb, nent);
  }
  patch_clear_guards<FR>(buf);
}

// XF: the held cells as the from-zero sweep of their rows, x = Jacobi(0; f), instead of a load of
// the vector the finer level's kernel would have stored: the expression of jacobi_from_zero_kernel
// and of the restriction loop below, operand for operand, on the f the thread holds anyway.  d = the
// diagonal of the cell's row type: the bits of the level's diagonal vector (the dictionary coding is
// exact; the sweeps divide by this very value) -- in scalar registers on a wave-uniform wave, else
// from the per-type table in global memory (utabd, 19 doubles per type: the LDS tables are not
// staged yet).  The absent type `ntypes` (rows outside the matrix, empty rows) has d = 0: x = 0.0.
template <class FR = PatchFrame>
__device__ __forceinline__ void patch_form_x(const PatchCells& pc, const PatchU& U,
                                             const double* __restrict__ utabd, double omega, double* buf) {
  double dv[PATCH_K];
  if (pc.uniform) {
#pragma unroll
    for (int k = 0; k < PATCH_K; ++k) dv[k] = U.diag;
  } else if (pc.coltyped) {  // one type per lane: one gather instead of PATCH_K
    const double d = utabd[(size_t)pc.lane_type() * 19 + 18];
#pragma unroll
    for (int k = 0; k < PATCH_K; ++k) dv[k] = d;
  } else {
#pragma unroll
    for (int k = 0; k < PATCH_K; ++k) dv[k] = utabd[(size_t)pc.type(k) * 19 + 18];
  }
#pragma unroll
  for (int k = 0; k < PATCH_K; ++k) {
    const double sum = pc.f[k], d = dv[k];
    const double xi = 0.0, acc = 0.0;  // jacobi_from_zero_kernel
    const double x0 = (d == 0.0) ? xi : xi + omega * ((sum - acc) / d - xi);
    buf[pc.cell0 + k * FR::EC] = pc.live[k] ? x0 : 0.0;
  }
}

// Everything a patch kernel does before its first barrier but the guards (patch_prologue): the loads
// of the tile, the row types, the uniform type's table and the cells' way into LDS.
// Every global load whose address does not hang on loaded data is ISSUED AT ENTRY, before anything
// is waited for, and waited for where its value is used:
//   x [-> uH pairs] -> f                          vector loads, in this order (they return in order)
//   tile flag -> the flagged type's table (U)     scalar loads, beside them
// so a workgroup of a flagged tile exposes ONE memory round trip before its first LDS write: the
// wait for x; f is first read inside the first stage and is not waited for before the first
// barrier.  The rows are the clamped ones of the general path -- the flag is not known yet; on a
// flagged tile every row is inside the matrix, so these are its own rows.
// The up-leg (PROLONG) holds x and the uH pairs, 48 registers, at entry and issues f as those
// retire into LDS: all three at once do not fit the 72 registers of four workgroups per CU.
// tf: the tile's flag (patch_flag of tflag[tile]; 255, or no tflag: no flag, rows of several types or
// outside the matrix), read once the tile is in flight -- a scalar wait is a wait for every scalar
// load, the kernel's arguments among them, so the flag's round trip must not stand before the
// tile's: every row of the patch and its halo has the row type tf (patch_tile_flags_kernel found that out
// at setup) -- no row-type loads, the wave-uniform path for all waves.  Only tf == 255 keeps
// dependent loads: the row types (what the flags were introduced to skip) with the per-lane
// tables beside them, then the table of the type a wave found uniform.
// PROLONG: the loaded vector is x + P uH (up-leg); else plain x.
// XF: x is not loaded and the cells are formed from f once the row type's diagonal is at hand
// (patch_form_x, called here).
// RINGS: the first held line is line -RINGS of the patch.
// (pc.f of a row outside the matrix is f[0]: such a cell is never `did`, its results are dropped.)
// ctype (the Jacobi legs and the seam; the multicolour kernel, !COLT, keeps the general path
// there): the column types of the tiles with flag 254 (patch_tile_flags_kernel).  On such a tile a thread
// reads ONE type byte, its column's, instead of PATCH_K row types, and the workgroup stages the slot-form
// tables of patch_eval_c instead of the per-entry ones.  A wave of such a tile whose lanes all have one
// type is `uniform` as on any tile.  Without ctype a flag 254 (none is built then) reads as 255.
template <int RINGS, bool PROLONG, bool XF = false, class FR = PatchFrame, bool COLT = true>
__device__ __forceinline__ void patch_load(PatchCells& pc, PatchU& U, const uint8_t* __restrict__ tflag,
                                           const uint8_t* __restrict__ ctype, int tile, int n, int m,
                                           int j0, int i0, const double* __restrict__ x,
                                           const double* __restrict__ f,
                                           const uint8_t* __restrict__ rtype, int ntypes,
                                           const double* __restrict__ uH, int nH,
                                           const double* __restrict__ ptab, int nent,
                                           const double* __restrict__ utabd,
                                           const int32_t* __restrict__ utabi, double omega, double* buf,
                                           PatchJ* tabJ, PatchR* tabR) {
  const int g = (int)threadIdx.x / FR::EC, col = (int)threadIdx.x - g * FR::EC;
  const int le = g * PATCH_K;            // first of the thread's PATCH_K consecutive lines
  pc.lj0 = le - RINGS;
  pc.li = col - FR::CL;
  pc.cell0 = (le + 1) * FR::EC + col;  // + 1: guard line
  const int64_t r0 = (int64_t)(j0 + pc.lj0) * m + i0 + pc.li;
  pc.row0 = (int)(r0 < -((int64_t)1 << 30) ? -((int64_t)1 << 30) : r0);
  double xv[PATCH_K];
  PatchPair pr[PATCH_K];
#pragma unroll
  for (int k = 0; k < PATCH_K; ++k) {
    const int64_t r64 = r0 + (int64_t)k * m;
    pc.live[k] = r64 >= 0 && r64 < (int64_t)n;
    if (!XF) xv[k] = x[pc.live[k] ? (int)r64 : 0];
  }
  if (PROLONG) {
#pragma unroll
    for (int k = 0; k < PATCH_K; ++k) {
      const int row = pc.row0 + k * m;
      const int j = pc.live[k] ? (row >> 1) : 0;
      // uH[j - 1] and uH[j] as ONE 16-byte load of the pair (jc - 1, jc), jc = j clamped to
      // [1, nH - 1] (nH >= 2 on a patch level): half the load instructions of two gathers
      const int jc = j < 1 ? 1 : (j > nH - 1 ? nH - 1 : j);
      pr[k] = *reinterpret_cast<const PatchPair*>(uH + (jc - 1));
    }
  }
  if (!PROLONG) {
#pragma unroll
    for (int k = 0; k < PATCH_K; ++k) {
      const int64_t r64 = r0 + (int64_t)k * m;
      pc.f[k] = f[pc.live[k] ? (int)r64 : 0];
    }
  }
  __builtin_amdgcn_sched_barrier(0);  // the tile is in flight before the flag is looked at
  const uint32_t tf = tflag ? patch_flag(tflag, tile) : PATCH_FLAG_GENERAL;
  const uint32_t nty = (uint32_t)ntypes;
  pc.flagged = tf < PATCH_FLAG_COLTYPED;
  pc.coltyped = COLT && ctype != nullptr && tf == PATCH_FLAG_COLTYPED;
  if (pc.flagged) {
    // (ty[] is not filled in -- type() does not read it: two registers less while the tile is in flight)
    pc.tu = tf;
    pc.uniform = true;
  } else if (pc.coltyped) {
    const uint32_t tl = (uint32_t)ctype[(int64_t)tile * FR::EC + col];  // (< ntypes: the flag kernel checked)
    // slot tables of every type and of the absent one: entry t = (type t / PATCH_CT, word t % PATCH_CT)
    const int t = (int)threadIdx.x, tt = t / PATCH_CT, tj = t - tt * PATCH_CT;
    const bool stage = t < (ntypes + 1) * PATCH_CT;  // (<= PATCH_MAXTAB / 5 * PATCH_CT < FR::NT)
    double vj = 0.0, vr = 0.0;
    if (stage) {
      vj = utabd[tt * 19 + (tj < 9 ? tj : 18)];
      vr = tj < 9 ? utabd[tt * 19 + 9 + tj] : __longlong_as_double((long long)(uint32_t)utabi[tt * 2]);
    }
    pc.ty[0] = tl;
    pc.ty[1] = 0;
    pc.tu = (uint32_t)__builtin_amdgcn_readfirstlane((int)tl);
    pc.uniform = __builtin_amdgcn_ballot_w64(tl != pc.tu) == 0;
    if (stage) {
      reinterpret_cast<double*>(tabJ)[t] = vj;
      reinterpret_cast<double*>(tabR)[t] = vr;
    }
  } else {
    PatchTabRow tb;
    patch_issue_tables(tb, ptab, nent);
    uint32_t mism = 0, ty[PATCH_K];
#pragma unroll
    for (int k = 0; k < PATCH_K; ++k) {
      const int64_t r64 = r0 + (int64_t)k * m;
      ty[k] = (uint32_t)rtype[pc.live[k] ? (int)r64 : 0];
    }
#pragma unroll
    for (int q = 0; q < PATCH_K / 4; ++q) pc.ty[q] = 0;
#pragma unroll
    for (int k = 0; k < PATCH_K; ++k) {
      ty[k] = (pc.live[k] && ty[k] < nty) ? ty[k] : nty;  // 255 = empty row -> absent row
      pc.ty[k >> 2] |= ty[k] << (8 * (k & 3));            // (nty < 256: the table holds (nty + 1) rows)
    }
    pc.tu = (uint32_t)__builtin_amdgcn_readfirstlane((int)ty[0]);
#pragma unroll
    for (int q = 0; q < PATCH_K / 4; ++q) mism |= pc.ty[q] ^ (pc.tu * 0x01010101u);
    pc.uniform = __builtin_amdgcn_ballot_w64(mism != 0) == 0 && pc.tu < nty;
    patch_stage_tables<FR>(tabJ, tabR, tb, nent);
  }
  {
    // (opaque from here on: else the compiler folds type() back into eight registers of tf, filled --
    // and in the up-leg spilled -- on the flagged path)
    int fl = (pc.flagged ? 1 : 0) | (pc.coltyped ? 2 : 0);
    asm("" : "+v"(fl));
    fl = __builtin_amdgcn_readfirstlane(fl);
    pc.flagged = (fl & 1) != 0;
    pc.coltyped = COLT && (fl & 2) != 0;
  }
  // the uniform type's table (scalar loads): on a flagged tile issued before the first vector wait
  patch_load_u(U, pc.uniform ? pc.tu : 0u, utabd, utabi);
  __builtin_amdgcn_sched_barrier(0);
  if (XF) patch_form_x<FR>(pc, U, utabd, omega, buf);
  if (PROLONG) {
    // j, jc and the rows of f are worked out again from here on: kept across the loads they cost
    // the registers that the 48 of x and the uH pairs need (the compiler would keep, then spill, them)
    int row0 = pc.row0;
    asm volatile("" : "+v"(row0));
    pc.row0 = row0;
  }
#pragma unroll
  for (int k = 0; k < PATCH_K && !XF; ++k) {
    const int row = pc.row0 + k * m;
    double x0 = pc.live[k] ? xv[k] : 0.0;
    if (PROLONG) {  // linear_prolong_add_kernel, same guards and order, written with selects
      const int j = pc.live[k] ? (row >> 1) : 0;
      const int jc = j < 1 ? 1 : (j > nH - 1 ? nH - 1 : j);
      const bool odd = (row & 1) != 0;
      const bool a_ok = pc.live[k] && !odd && j >= 1 && j - 1 < nH;
      const bool b_ok = pc.live[k] && j < nH;
      const double a = (j == jc) ? pr[k].x : pr[k].y;   // j - 1 == jc - 1, or j - 1 == jc (j == nH)
      const double b = (j == jc) ? pr[k].y : pr[k].x;   // j == jc, or j == jc - 1 (j == 0)
      double t = 0.0;
      t = a_ok ? t + 0.5 * a : t;
      t = b_ok ? t + (odd ? 1.0 : 0.5) * b : t;
      x0 = pc.live[k] ? x0 + t : x0;
    }
    buf[pc.cell0 + k * FR::EC] = x0;
  }
  if (PROLONG) {
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < PATCH_K; ++k) pc.f[k] = f[pc.live[k] ? pc.row0 + k * m : 0];  // (a live row is row0 + k m)
  }
}

// flag[tile] = the row type shared by EVERY row a patch kernel of `rings` rings loads for the tile
// (lines -rings .. TH+rings, columns -4 .. TW+4 of the flat index, all inside the matrix), else 255.
// (eh, ec: the held frame, columns -(ec - TW) / 2 .. of the flat index: that of the legs, or the seam kernel's)
// ctype (optional): a tile that is not of one type but whose every held row is inside the matrix and whose
// every held COLUMN has one row type over all eh lines (the tiles at the line ends, away from the first
// and last lines) gets the flag PATCH_FLAG_COLTYPED, and ctype[tile * ec + c] = the type of held column c.
__global__ __launch_bounds__(256) void patch_tile_flags_kernel(int n, int m, int px_count, int rings, int eh, int ec,
                                                               const uint8_t* __restrict__ rtype,
                                                               int ntypes, uint8_t* __restrict__ flag,
                                                               uint8_t* __restrict__ ctype) {
  const int tile = blockIdx.x;
  const int py = tile / px_count, px = tile - py * px_count;
  const int64_t base = (int64_t)(py * (eh - 2 * rings) - rings) * m + px * PATCH_TW - (ec - PATCH_TW) / 2;
  const int64_t first = base < 0 ? 0 : (base < n ? base : n - 1);
  const uint32_t t0 = rtype[first];
  int ok = base >= 0 && t0 < (uint32_t)ntypes;
  int okc = base >= 0 && base + (int64_t)(eh - 1) * m + ec <= (int64_t)n;  // every held row is inside the matrix
  for (int q = threadIdx.x; q < eh * ec; q += 256) {
    const int le = q / ec, c = q - le * ec;
    const int64_t r = base + (int64_t)le * m + c;
    const uint32_t t = rtype[r < 0 ? 0 : (r < n ? r : n - 1)];
    ok = ok && r >= 0 && r < (int64_t)n && t == t0;
    if (okc) {
      const uint32_t tc = rtype[base + c];  // the column's type on the first held line
      okc = tc < (uint32_t)ntypes && t == tc;
    }
  }
  ok = __syncthreads_and(ok);
  okc = __syncthreads_and(okc) && ctype != nullptr;
  if (threadIdx.x == 0)
    flag[tile] = ok ? (uint8_t)t0 : (okc ? (uint8_t)PATCH_FLAG_COLTYPED : (uint8_t)PATCH_FLAG_GENERAL);
  if (!ok && okc && (int)threadIdx.x < ec) ctype[(int64_t)tile * ec + threadIdx.x] = rtype[base + threadIdx.x];
}
int patch_frame_columns(int rings) { return rings == PATCH_SEAM_RINGS_HOST ? 76 : PATCH_EC; }
hipError_t launch_patch_tile_flags(int64_t n, int64_t m, int rings, const uint8_t* rtype, int ntypes,
                                   uint8_t* flag, int64_t* n_tiles, hipStream_t st, uint8_t* ctype) {
  if (!patch_geometry_ok(n, m) || !patch_rings_ok(rings)) return hipErrorInvalidValue;
  const int64_t lines = (n + m - 1) / m;
  const int pxc = (int)(m / PATCH_TW);
  const int64_t th = patch_th(rings);
  const int64_t tiles = (lines + th - 1) / th * pxc;
  if (n_tiles) *n_tiles = tiles;
  if (!flag) return hipSuccess;
  hipLaunchKernelGGL(patch_tile_flags_kernel, dim3((unsigned)tiles), dim3(256), 0, st, (int)n, (int)m, pxc,
                     rings, PATCH_EH, PATCH_EC, rtype, ntypes, flag,
                     ntypes < (int)PATCH_FLAG_COLTYPED ? ctype : nullptr);  // (the flag values 254, 255 are no types)
  return hipGetLastError();
}

// cflag[tile] = 1 when every coarse row the down-leg of the tile (th lines) produces (c = i / 2 for
// the even fine rows i of the patch) has the diagonal dref, bit for bit.
__global__ __launch_bounds__(256) void patch_coarse_flags_kernel(int n, int m, int px_count, int th, int nH,
                                                                 const double* __restrict__ diagH, double dref,
                                                                 uint8_t* __restrict__ cflag) {
  const int tile = blockIdx.x;
  const int py = tile / px_count, px = tile - py * px_count;
  const int j0 = py * th, i0 = px * PATCH_TW;
  int ok = 1;
  for (int q = threadIdx.x; q < th * (PATCH_TW / 2); q += 256) {
    const int lj = q / (PATCH_TW / 2), cx = q - lj * (PATCH_TW / 2);
    const int64_t i = (int64_t)(j0 + lj) * m + i0 + 2 * cx;
    const int64_t c = i >> 1;
    if (i >= (int64_t)n || c >= nH) continue;
    ok = ok && __double_as_longlong(diagH[c]) == __double_as_longlong(dref);
  }
  ok = __syncthreads_and(ok);
  if (threadIdx.x == 0) cflag[tile] = ok ? 1 : 0;
}
hipError_t launch_patch_coarse_flags(int64_t n, int64_t m, int rings, int64_t nH, const double* diagH,
                                     double dref, uint8_t* cflag, hipStream_t st) {
  if (!patch_geometry_ok(n, m) || !patch_rings_ok(rings) || !diagH || !cflag) return hipErrorInvalidValue;
  const int64_t lines = (n + m - 1) / m;
  const int pxc = (int)(m / PATCH_TW);
  const int64_t th = patch_th(rings);
  const int64_t tiles = (lines + th - 1) / th * pxc;
  hipLaunchKernelGGL(patch_coarse_flags_kernel, dim3((unsigned)tiles), dim3(256), 0, st, (int)n, (int)m, pxc,
                     (int)th, (int)nH, diagH, dref, cflag);
  return hipGetLastError();
}

// FIRST: the input is the level's u and both pre-sweeps run here (level 0); else the input
// is the result of the first sweep (done by the finer level's kernel) and one sweep runs.
// XF (with !FIRST): that first sweep is not loaded but formed from f (patch_form_x); the finer
// level's kernel then was launched with uH1 == nullptr and stored f_H only.
// (Tried and dropped: at most 1024 workgroups per launch, each walking several patches of its XCD's
// run with the tables staged once -- the loop alone cost 20 % (165 vs 134 us on level 0), with
// 1024 workgroups 204 us: the slots of a CU standing empty 40 % of the time
// (SQ_WAVE_CYCLES / (slots x duration) = 0.59) is not workgroup turnover.)
#ifdef AMG_PATCH_STAMPS
// DIAGNOSTIC BUILD ONLY (never shipped, never timed): per workgroup the 100 MHz wall clock at the
// phase boundaries of the down-leg and the hardware id of the CU it ran on, into a buffer of its
// own (tools/patch_stamps.py reads it: phase shares, workgroups resident per CU, dispatch gaps).
// g_patch_stamps_rows != 0: only the launches on a level of that many rows leave stamps (one leg out
// of a whole cycle).  Slot 6: (flag-array index of the tile << 8) | its flag as the kernel read it.
__device__ unsigned long long* g_patch_stamps = nullptr;
__device__ int g_patch_stamps_rows = 0;
__device__ __forceinline__ void patch_stamp_flag(int n, int ftile, uint32_t tf) {
  if (threadIdx.x == 0 && g_patch_stamps && (g_patch_stamps_rows == 0 || g_patch_stamps_rows == n))
    g_patch_stamps[(size_t)blockIdx.x * 8 + 6] = ((unsigned long long)(unsigned)ftile << 8) | (tf & 255u);
}
__device__ __forceinline__ void patch_stamp(int k, int n) {
  if (threadIdx.x == 0 && g_patch_stamps && (g_patch_stamps_rows == 0 || g_patch_stamps_rows == n)) {
    unsigned long long t = __builtin_amdgcn_s_memrealtime();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    g_patch_stamps[(size_t)blockIdx.x * 8 + k] = t;
    if (k == 0) {
      const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | 4);    // HW_REG_HW_ID
      const unsigned xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20);   // HW_REG_XCC_ID
      g_patch_stamps[(size_t)blockIdx.x * 8 + 7] = ((unsigned long long)xcc << 32) | hw;
    }
  }
}
hipError_t debug_set_patch_stamps(unsigned long long* p) {
  return hipMemcpyToSymbol(HIP_SYMBOL(g_patch_stamps), &p, sizeof(p));
}
hipError_t debug_set_patch_stamps_rows(int rows) {
  return hipMemcpyToSymbol(HIP_SYMBOL(g_patch_stamps_rows), &rows, sizeof(rows));
}
#define PATCH_STAMP(k) patch_stamp(k, n)
#define PATCH_STAMP_FLAG(ftile, tf) patch_stamp_flag(n, ftile, tf)
#else
#define PATCH_STAMP(k)
#define PATCH_STAMP_FLAG(ftile, tf)
#endif
template <int UN, int UM, bool FIRST, bool NT, bool XF = false, int RINGS = 3>
// (four workgroups per CU = 7 waves per SIMD = 72 registers: measured against 6 and 5 waves again in
// round 3 -- level-0 down-leg 131-135 us at 7, 138-144 at 6, 142-143 at 5.  The down-legs of the
// 7- and 9-point levels spill 2-7 registers at 72 and run at 6 waves (80 registers, three
// workgroups per CU): cycle 1288 / 1290 / 1291 -> 1315 / 1305 / 1308 V-cycles/s in alternating runs;
// their up-legs, which fit, stay at 7: 1296 / 1298 with both at 6.
// The XF variants hold no xv[8] while loading, but the peak is in the stages: compiled at 72 the
// 7- and 9-point XF kernels still spill 7-8 registers (20-24 B of scratch per lane; the stored
// form: 4-12 registers, 12-28 B), so they do not fit 7 waves either and stay at 6, where the
// compiler reports 80 registers and 24-28 B of scratch for XF against 20-24 B for the stored form
// (7-point: none for both).  The 5-point XF kernel fits 72 without scratch, like the stored form.)
#ifndef AMG_PATCH_WAVES
#define AMG_PATCH_WAVES 7
#endif
__global__ __launch_bounds__(PATCH_NT, (UN == 5 ? AMG_PATCH_WAVES : AMG_PATCH_WAVES - 1)) void patch_down_kernel(
    int n, int m, int px_count, const uint8_t* __restrict__ rtype, const double* __restrict__ ptab,
    const double* __restrict__ utabd, const int32_t* __restrict__ utabi,
    int nent, int ntypes, const double* x, const double* __restrict__ f, double* u_out, double* r_out, int nH,
    double* __restrict__ fH, const double* __restrict__ diagH, double* __restrict__ uH1,
    double omega, int xcd_map, int py0, const uint8_t* __restrict__ tflag,
    const uint8_t* __restrict__ cflag, double dHu, const uint8_t* __restrict__ ctype) {
  __shared__ double buf[PATCH_BUF];
  __shared__ PatchJ tabJ[PATCH_MAXTAB];
  __shared__ PatchR tabR[PATCH_MAXTAB];
  PATCH_STAMP(0);
  const int tile = xcd_tile(blockIdx.x, gridDim.x, xcd_map);
  const int py = tile / px_count, px = tile - py * px_count;
  constexpr int TH = patch_th(RINGS);
  const int j0 = (py + py0) * TH, i0 = px * PATCH_TW;
  PatchCells pc;
  PatchU U;
  const int ftile = (py + py0) * px_count + px;
  static_assert(!(FIRST && XF), "level 0 starts from its own u");
  static_assert(RINGS == 3 || (RINGS == 2 && !FIRST), "three dependent stages (FIRST) need three rings");
  // (the 5-point kind keeps the general path on column-typed tiles: patch_eval_c's note)
  patch_load<RINGS, false, XF, PatchFrame, UN != 5>(pc, U, tflag, ctype, ftile, n, m, j0, i0, x, f, rtype, ntypes, nullptr, 0, ptab, nent,
                               utabd, utabi, omega, buf, tabJ, tabR);
  patch_prologue<UM>(pc, U, buf, tabJ, tabR, ptab, nent);
  // every coarse row under this patch has the diagonal dHu (launch_patch_coarse_flags found that
  // out at setup): the first coarse sweep then needs no load of the coarse diagonal at the very
  // end of the workgroup's life, where nothing is left to hide its latency behind.  (A scalar load
  // like the tile flag's, issued behind the tile; read in the restriction loop.)
  const bool cuni = uH1 && cflag && patch_flag(cflag, ftile) != 0;
  lds_barrier();
  PATCH_STAMP(1);
  PATCH_STAMP_FLAG(ftile, pc.flagged ? pc.tu : (pc.coltyped ? PATCH_FLAG_COLTYPED : PATCH_FLAG_GENERAL));
  if (FIRST) {
    patch_stage<UN, UM, false, NT, false, TH>(pc, m, ntypes, buf, U, tabJ, tabR, omega, -2, TH + 2, -2,
                                              PATCH_TW + 3, nullptr);
    lds_barrier();
  }
  PATCH_STAMP(2);
  patch_stage<UN, UM, false, NT, false, TH>(pc, m, ntypes, buf, U, tabJ, tabR, omega, -1, TH + 1, -1,
                                            PATCH_TW + 2, nullptr);
  lds_barrier();
  PATCH_STAMP(3);
  patch_copy_out<NT, RINGS>(buf, u_out, n, m, j0, i0);  // the residual stage below only reads until its barrier
  // residual; rows outside the matrix read as 0.0 for the restriction (ZERO)
  patch_stage<UN, UM, true, NT, true, TH>(pc, m, ntypes, buf, U, tabJ, tabR, omega, 0, TH, 0, PATCH_TW + 1,
                                          r_out);
  lds_barrier();
  PATCH_STAMP(4);
  const double* rsb = buf;
  // restriction + first coarse sweep: coarse row c <-> even fine row 2c of the patch
  // (uH1 == nullptr: the coarse level's kernel forms that sweep from f_H itself -- XF -- and f_H
  // alone is stored: no coarse diagonal, no division)
  for (int q = threadIdx.x; q < TH * (PATCH_TW / 2); q += PATCH_NT) {
    const int lj = q / (PATCH_TW / 2), cx = q - lj * (PATCH_TW / 2);
    const int64_t i = (int64_t)(j0 + lj) * m + i0 + 2 * cx;   // fine row 2c
    const int64_t c = i >> 1;
    if (i >= (int64_t)n || c >= nH) continue;
    const double* rs = rsb + (lj + RINGS + 1) * PATCH_EC + 2 * cx + 4;
    double sum = 0.0;  // dict_restrict_tail / linear_restrict_kernel, same guards and order
    if (i < n) sum += 0.5 * rs[0];
    if (i + 1 < n) sum += 1.0 * rs[1];
    if (i + 2 < n) sum += 0.5 * rs[2];
    fH[c] = sum;
    if (uH1 == nullptr) continue;
    const double xi = 0.0, acc = 0.0;  // jacobi_from_zero_kernel
    const double d = cuni ? dHu : diagH[c];
    uH1[c] = (d == 0.0) ? xi : xi + omega * ((sum - acc) / d - xi);
  }
  PATCH_STAMP(5);
}

template <int UN, int UM, bool NT, int RINGS = 3>
__global__ __launch_bounds__(PATCH_NT, AMG_PATCH_WAVES) void patch_up_kernel(
    int n, int m, int px_count, const uint8_t* __restrict__ rtype, const double* __restrict__ ptab,
    const double* __restrict__ utabd, const int32_t* __restrict__ utabi,
    int nent, int ntypes, const double* x, const double* __restrict__ f, const double* __restrict__ uH, int nH,
    double* u_out, double omega, int xcd_map, int py0, const uint8_t* __restrict__ tflag,
    const uint8_t* __restrict__ ctype) {
  __shared__ double buf[PATCH_BUF];
  __shared__ PatchJ tabJ[PATCH_MAXTAB];
  __shared__ PatchR tabR[PATCH_MAXTAB];
  const int tile = xcd_tile(blockIdx.x, gridDim.x, xcd_map);
  const int py = tile / px_count, px = tile - py * px_count;
  static_assert(RINGS == 2 || RINGS == 3, "two dependent stages");
  constexpr int TH = patch_th(RINGS);
  const int j0 = (py + py0) * TH, i0 = px * PATCH_TW;
  PatchCells pc;
  PatchU U;
  patch_load<RINGS, true>(pc, U, tflag, ctype, (py + py0) * px_count + px, n, m, j0, i0, x, f, rtype, ntypes, uH, nH,
                          ptab, nent, utabd, utabi, omega, buf, tabJ, tabR);
  patch_prologue<UM>(pc, U, buf, tabJ, tabR, ptab, nent);
  lds_barrier();
  patch_stage<UN, UM, false, NT, false, TH, PatchFrame, true>(pc, m, ntypes, buf, U, tabJ, tabR, omega, -1, TH + 1, -1,
                                                              PATCH_TW + 1, nullptr);
  lds_barrier();
  patch_stage<UN, UM, false, NT, false, TH, PatchFrame, true>(pc, m, ntypes, buf, U, tabJ, tabR, omega, 0, TH, 0,
                                                              PATCH_TW, nullptr);
  lds_barrier();
  patch_copy_out<NT, RINGS>(buf, u_out, n, m, j0, i0);
}

// The seam between two cycles on level 0: the up-leg of cycle k and the down-leg of cycle k + 1 in ONE
// launch, on one loaded tile -- x = u + P u_H (patch_load, the up-leg's), post-sweep 1, post-sweep 2,
// pre-sweep 1, pre-sweep 2 (stored), residual, restriction (f_H alone: level 1 forms its first sweep
// from it, the uH1 == nullptr form of the down-leg).  The vector u between the two legs is neither
// stored nor loaded, f and the row types are read once.  Five dependent stencil stages: five rings
// of halo lines, and columns [-5, TW + 6) -- the frame FR (columns [-6, TW + 6)).  Every stage is
// the legs' own patch_stage on the legs' regions grown by the rings still to come, so every value
// has the bits the two launches give it (halo cells are recomputed, as everywhere in K-Patch).
constexpr int PATCH_SEAM_RINGS = 5;
static_assert(PATCH_SEAM_RINGS == PATCH_SEAM_RINGS_HOST, "patch_frame_columns");
template <int UN, int UM, bool NT, class FR, int WAVES>
__global__ __launch_bounds__(FR::NT, WAVES) void patch_seam_kernel(
    int n, int m, int px_count, const uint8_t* __restrict__ rtype, const double* __restrict__ ptab,
    const double* __restrict__ utabd, const int32_t* __restrict__ utabi,
    int nent, int ntypes, const double* x, const double* __restrict__ f, const double* __restrict__ uH, int nH,
    double* u_out, double* __restrict__ fH, double omega, int xcd_map, const uint8_t* __restrict__ tflag,
    const uint8_t* __restrict__ ctype) {
  __shared__ double buf[FR::BUF];
  __shared__ PatchJ tabJ[PATCH_MAXTAB];
  __shared__ PatchR tabR[PATCH_MAXTAB];
  const int tile = xcd_tile(blockIdx.x, gridDim.x, xcd_map);
  const int py = tile / px_count, px = tile - py * px_count;
  constexpr int RINGS = PATCH_SEAM_RINGS, TH = FR::th(RINGS);
  static_assert(TH >= 1 && FR::CL >= RINGS + 1, "five stages and the restriction's column");
  const int j0 = py * TH, i0 = px * PATCH_TW;
  PatchCells pc;
  PatchU U;
  patch_load<RINGS, true, false, FR>(pc, U, tflag, ctype, tile, n, m, j0, i0, x, f, rtype, ntypes, uH, nH, ptab, nent,
                                     utabd, utabi, omega, buf, tabJ, tabR);
  patch_prologue<UM, FR>(pc, U, buf, tabJ, tabR, ptab, nent);
  lds_barrier();
#pragma unroll
  for (int q = 4; q >= 1; --q) {  // post-sweeps 1, 2, pre-sweeps 1, 2: q rings are still to come
    patch_stage<UN, UM, false, NT, false, TH, FR>(pc, m, ntypes, buf, U, tabJ, tabR, omega, -q, TH + q, -q,
                                                  PATCH_TW + q + 1, nullptr);
    lds_barrier();
  }
  patch_copy_out<NT, RINGS, FR>(buf, u_out, n, m, j0, i0);  // the residual stage below only reads until its barrier
  patch_stage<UN, UM, true, NT, true, TH, FR>(pc, m, ntypes, buf, U, tabJ, tabR, omega, 0, TH, 0, PATCH_TW + 1,
                                              nullptr);
  lds_barrier();
  for (int q = threadIdx.x; q < TH * (PATCH_TW / 2); q += FR::NT) {  // patch_down_kernel's loop, f_H alone
    const int lj = q / (PATCH_TW / 2), cx = q - lj * (PATCH_TW / 2);
    const int64_t i = (int64_t)(j0 + lj) * m + i0 + 2 * cx;   // fine row 2c
    const int64_t c = i >> 1;
    if (i >= (int64_t)n || c >= nH) continue;
    const double* rs = buf + (lj + RINGS + 1) * FR::EC + 2 * cx + FR::CL;
    double sum = 0.0;  // dict_restrict_tail / linear_restrict_kernel, same guards and order
    if (i < n) sum += 0.5 * rs[0];
    if (i + 1 < n) sum += 1.0 * rs[1];
    if (i + 2 < n) sum += 0.5 * rs[2];
    fH[c] = sum;
  }
}

// ---- multicolour Gauss-Seidel on a patch (colours laid out on the 2 x 2 cells of the grid) ----
// One colour of a Gauss-Seidel half-sweep as a patch stage: cells of colour `c` inside the
// region take (f - sum of off-diagonal terms) / diagonal from the CURRENT neighbours (which all
// have other colours), every other cell keeps its value.  cbits: bits 2k, 2k+1 = colour of cell k.
template <int UN, int UM>
__device__ __forceinline__ void patch_stage_color(const PatchCells& pc, int ntypes, double* buf,
                                                  const PatchU& U, const PatchJ* tabJ, const PatchR* tabR,
                                                  int l0, int l1, int c0, int c1, uint32_t cbits,
                                                  uint32_t c) {
  const bool inc = pc.li >= c0 && pc.li < c1;
  double res[PATCH_K];
  bool did[PATCH_K];
#pragma unroll
  for (int k = 0; k < PATCH_K; ++k) {
    const int lj = pc.lj0 + k;
    did[k] = inc && lj >= l0 && lj < l1 && pc.live[k] && ((cbits >> (2 * k)) & 3u) == c;
  }
  // A wave none of whose cells has the stage's colour has nothing to do (the colours of the line
  // ends on level 1: almost every wave; -9 % on that level).  Otherwise every cell is evaluated and
  // the other colours' results are dropped: evaluating only the lines that hold the colour (every
  // other one, for the colourings by lines and by products) was measured no faster -- a stage is
  // bound by its LDS round trips and barriers, not by the arithmetic -- and any finer branching
  // (a ballot per cell) 35 % slower.
  bool any = false;
#pragma unroll
  for (int k = 0; k < PATCH_K; ++k) any |= did[k];
  if (__builtin_amdgcn_ballot_w64(any) == 0) return;
  if (pc.uniform && U.rmask == (uint32_t)UM) {
    constexpr bool CN = (UM & 0x145) != 0;
    constexpr int MK = (UM & 0x145) ? -1 : UM;
    patch_eval_u<false, CN, true, MK>(buf, pc.cell0, U, pc.f, 1.0, res);
  } else {
#pragma unroll
    for (int k = 0; k < PATCH_K; ++k)
      res[k] = patch_eval<UN, false, true>(buf, pc.cell0 + k * PATCH_EC,
                                           did[k] ? pc.type(k) : (uint32_t)ntypes, tabJ, tabR, pc.f[k], 1.0);
  }
  // cells of one colour do not read each other: no barrier between the reads and the writes
#pragma unroll
  for (int k = 0; k < PATCH_K; ++k)
    if (did[k]) buf[pc.cell0 + k * PATCH_EC] = res[k];
}

// Up to three colour stages on the loaded patch -- a piece of the symmetric pass 0 .. nc-1, nc-1 .. 0
// (a colour that directly follows itself is dropped by the host: its rows read no row of their own
// colour, so the repeat would write the bits that are already there) -- in the frame of the Jacobi
// kernels above:
//   !TAIL: like the up-leg: [u + P u_H while loading when PROLONG], up to 3 stages, store;
//    TAIL: like the level-0 down-leg: up to 2 stages, store, residual, restriction (f_H; the
//          coarse u is zeroed, multigrid.hpp:278).
// stages: bits 0-2 = number of stages, bits 4+2s, 5+2s = colour of stage s.
// colour(row) = ctab entry (line & 1) * 6 + column class, 2 bits each; column classes: 0, 1, m-2,
// m-1 (the line ends, whose rows differ) and the even / odd columns between them (what the greedy
// colouring yields on these stencils: the checkerboard on the 5-point level; line parity with
// colours of their own at the line ends on level 1, where only the lines above and below are
// coupled; the product colouring on the 9-point levels -- verified on the host against the
// colouring itself).  Same row arithmetic as the colour kernels
// (dict_rows<CSR_GS>): ascending-column sum of the off-diagonal terms, IEEE divide.
template <int UN, int UM, bool NT, bool PROLONG, bool TAIL>
// (Register budget: with the stage loop, the colour bits and the residual stage the kernel does not
// fit the 72 registers of four workgroups per CU -- 26-118 spilled registers, and the scratch
// traffic showed as 1.6x the write bytes in the PMC record.  At 96 registers (two workgroups per
// CU) nothing spills: 8192^2 multicolour 190.9 -> 203.2 V-cycles/s, 4096^2 576.9 -> 607.0; three
// workgroups / 80 registers: 196.5 / 593.1.  The Jacobi kernels, which fit 72, are fastest at four.)
#ifndef AMG_RB_WAVES
#define AMG_RB_WAVES 5
#endif
__global__ __launch_bounds__(PATCH_NT, AMG_RB_WAVES) void patch_rb_kernel(
    int n, int m, int px_count, const uint8_t* __restrict__ rtype, const double* __restrict__ ptab,
    const double* __restrict__ utabd, const int32_t* __restrict__ utabi, int nent, int ntypes,
    const double* x, const double* __restrict__ f, const double* __restrict__ uH, int nH, double* u_out,
    double* r_out, double* __restrict__ fH, double* __restrict__ uH_zero, uint32_t stages, uint32_t ctab,
    int xcd_map, int py0, const uint8_t* __restrict__ tflag) {
  __shared__ double buf[PATCH_BUF];
  __shared__ PatchJ tabJ[PATCH_MAXTAB];
  __shared__ PatchR tabR[PATCH_MAXTAB];
  const int tile = xcd_tile(blockIdx.x, gridDim.x, xcd_map);
  const int py = tile / px_count, px = tile - py * px_count;
  constexpr int RINGS = 3, TH = patch_th(RINGS);  // up to three dependent stages
  const int j0 = (py + py0) * TH, i0 = px * PATCH_TW;
  PatchCells pc;
  PatchU U;
  patch_load<RINGS, PROLONG, false, PatchFrame, false>(pc, U, tflag, nullptr, (py + py0) * px_count + px, n, m, j0, i0, x, f, rtype, ntypes, uH, nH,
                             ptab, nent, utabd, utabi, 1.0, buf, tabJ, tabR);
  patch_prologue<UM>(pc, U, buf, tabJ, tabR, ptab, nent);
  uint32_t cbits = 0;
  {
    // the cell is flat row (j0 + lj) * m + i0 + li: beyond a line's end that is a row of the next / previous line
    const int col = i0 + pc.li;
    const uint32_t line = (uint32_t)(j0 + pc.lj0 + (col < 0 ? -1 : (col >= m ? 1 : 0)) + 64);
    const int tc = col < 0 ? col + m : (col >= m ? col - m : col);
    const uint32_t cls = tc == 0 ? 0u : (tc == 1 ? 1u : (tc == m - 2 ? 2u : (tc == m - 1 ? 3u : 4u + ((uint32_t)tc & 1u))));
#pragma unroll
    for (int k = 0; k < PATCH_K; ++k)
      cbits |= ((ctab >> (2u * (((line + (uint32_t)k) & 1u) * 6u + cls))) & 3u) << (2 * k);
  }
  lds_barrier();
  if (pc.flagged) pc.ty[0] = pc.ty[1] = 0;  // (not read; defined for the asm in the loop below)
  constexpr int E = TAIL ? 1 : 0;  // the residual stage needs one more ring (and the restriction one more column)
  const int nst = (int)(stages & 7u);
  for (int sg = 0; sg < nst; ++sg) {
    const int ext = nst - 1 - sg + E;  // rings the later stages still read
    // (the packed row types are unpacked at their use: hoisted out of this loop the bytes cost eight
    // registers again, and the kernel spills)
    asm volatile("" : "+v"(pc.ty[0]), "+v"(pc.ty[1]));
    patch_stage_color<UN, UM>(pc, ntypes, buf, U, tabJ, tabR, -ext, TH + ext, -ext, PATCH_TW + ext + E,
                              cbits, (stages >> (4 + 2 * sg)) & 3u);
    lds_barrier();
  }
  patch_copy_out<NT, RINGS>(buf, u_out, n, m, j0, i0);
  if (TAIL) {
    patch_stage<UN, UM, true, NT, true, TH>(pc, m, ntypes, buf, U, tabJ, tabR, 1.0, 0, TH, 0, PATCH_TW + 1,
                                            r_out);
    lds_barrier();
    for (int q = threadIdx.x; q < TH * (PATCH_TW / 2); q += PATCH_NT) {
      const int lj = q / (PATCH_TW / 2), cx = q - lj * (PATCH_TW / 2);
      const int64_t i = (int64_t)(j0 + lj) * m + i0 + 2 * cx;   // fine row 2c
      const int64_t c = i >> 1;
      if (i >= (int64_t)n || c >= nH) continue;
      const double* rs = buf + (lj + RINGS + 1) * PATCH_EC + 2 * cx + 4;
      double sum = 0.0;  // dict_restrict_tail / linear_restrict_kernel, same guards and order
      if (i < n) sum += 0.5 * rs[0];
      if (i + 1 < n) sum += 1.0 * rs[1];
      if (i + 2 < n) sum += 0.5 * rs[2];
      fH[c] = sum;
      if (uH_zero) uH_zero[c] = 0.0;  // multigrid.hpp:278
    }
  }
}
int patch_un(int un) { return un <= 5 ? 5 : un <= 7 ? 7 : 9; }
bool patch_geometry_ok(int64_t n, int64_t m) {
  return m >= 2 * PATCH_TW && (m % PATCH_TW) == 0 && n >= m && n < ((int64_t)1 << 31) - 4 * m - 64;
}
// tiles (of th lines) that meet the lines [line_lo, line_hi) (line_hi < 0: all); *py0 = first tile row
static unsigned patch_grid(int64_t n, int64_t m, int th, int64_t line_lo, int64_t line_hi, int* px_count,
                           int* py0) {
  const int64_t lines = (n + m - 1) / m;
  if (line_hi < 0 || line_hi > lines) line_hi = lines;
  if (line_lo < 0) line_lo = 0;
  if (line_lo > line_hi) line_lo = line_hi;
  *px_count = (int)(m / PATCH_TW);
  *py0 = (int)(line_lo / th);
  return (unsigned)(((line_hi + th - 1) / th - *py0) * *px_count);
}
int patch_tile_lines(int rings) { return patch_rings_ok(rings) ? patch_th(rings) : 0; }
// THE choice of a Jacobi leg's geometry where tall legs are on: the level-0 down-leg (first) runs
// three dependent stages on the loaded data, every other leg two.  (A kernel kind that came out
// slower on 44 lines than on 42 would be kept on three rings here.)
int patch_leg_rings(bool first) { return first ? 3 : 2; }
// kernel kinds: (row width of the per-lane path, slots of the interior row type -- the scalar path)
//   (5, 0x0BA) the 5-point level 0; (7, 0x1D7) / (9, 0x1D7) level 1, whose +-1 entries are exact
//   zeros and pruned (its line ends keep rows of 9); (9, 0x1FF) the 9-point levels
int patch_default_umask(int un) { return un <= 5 ? 0x0BA : (un <= 7 ? 0x1D7 : 0x1FF); }
// the mask of the kernel kind patch_dispatch picks for (un, umask)
int patch_kind_umask(int un, int umask) { return (un > 7 && un <= 9 && umask == 0x1D7) ? 0x1D7 : patch_default_umask(un); }
template <class F>
static hipError_t patch_dispatch(int un, int umask, bool nt, F&& go) {
  using std::integral_constant;
  auto with_nt = [&](auto U, auto M) {
    if (nt) go(U, M, integral_constant<bool, true>{});
    else go(U, M, integral_constant<bool, false>{});
  };
  if (un <= 5) with_nt(integral_constant<int, 5>{}, integral_constant<int, 0x0BA>{});
  else if (un <= 7) with_nt(integral_constant<int, 7>{}, integral_constant<int, 0x1D7>{});
  else if (un <= 9 && umask == 0x1D7) with_nt(integral_constant<int, 9>{}, integral_constant<int, 0x1D7>{});
  else if (un <= 9) with_nt(integral_constant<int, 9>{}, integral_constant<int, 0x1FF>{});
  else return hipErrorInvalidValue;
  return hipGetLastError();
}
hipError_t launch_patch_down(bool first, int64_t n, int64_t m, const PatchRef& P, const double* x,
                             const double* f, double* u_out, double* r_out, int64_t nH, double* fH,
                             const double* diagH, double* uH1, double omega, hipStream_t st,
                             int64_t line_lo, int64_t line_hi, bool xf) {
  // uH1 == nullptr: f_H only (the coarse level runs the xf form); xf: x is formed from f, not read
  if (!patch_geometry_ok(n, m) || !P.rtype || !P.ptab || !P.utabd || !P.utabi || (P.ntypes + 1) * patch_un(P.un) > PATCH_MAXTAB ||
      P.nent != P.ntypes * patch_un(P.un) || !fH || (uH1 && !diagH) || !u_out || u_out == x || (xf ? first : !x) ||
      !patch_rings_ok(P.rings) || P.rings < patch_leg_rings(first))
    return hipErrorInvalidValue;
  // P.rings is the geometry of everything below: the tile grid, py0, the flags P carries, the kernel
  int pxc = 0, py0 = 0;
  const unsigned grid = patch_grid(n, m, patch_th(P.rings), line_lo, line_hi, &pxc, &py0);
  if (grid == 0) return hipSuccess;
  const int xm = g_xcd_map ? 1 : 0;  // halo lines of neighbouring patches meet in one L2
  return patch_dispatch(P.un, P.umask, P.nt != 0, [&](auto U, auto M, auto NTF) {
#define AMG_DOWN(FST, XFF, RG)                                                                                 \
  hipLaunchKernelGGL((patch_down_kernel<decltype(U)::value, decltype(M)::value, FST, decltype(NTF)::value, XFF, RG>), \
                     dim3(grid), dim3(PATCH_NT), 0, st, (int)n, (int)m, pxc, P.rtype, P.ptab, P.utabd, P.utabi, \
                     P.nent, P.ntypes, x, f, u_out, r_out, (int)nH, fH, diagH, uH1, omega, xm, py0, P.tflag,    \
                     P.cflag, P.dHu, P.ctype)
    if (first) AMG_DOWN(true, false, 3);
    else if (xf && P.rings == 2) AMG_DOWN(false, true, 2);
    else if (xf) AMG_DOWN(false, true, 3);
    else if (P.rings == 2) AMG_DOWN(false, false, 2);
    else AMG_DOWN(false, false, 3);
#undef AMG_DOWN
  });
}
hipError_t launch_patch_up(int64_t n, int64_t m, const PatchRef& P, const double* x, const double* f,
                           const double* uH, int64_t nH, double* u_out, double omega,
                           hipStream_t st, int64_t line_lo, int64_t line_hi) {
  if (!patch_geometry_ok(n, m) || !P.rtype || !P.ptab || !P.utabd || !P.utabi || (P.ntypes + 1) * patch_un(P.un) > PATCH_MAXTAB ||
      P.nent != P.ntypes * patch_un(P.un) || !uH || !u_out || u_out == x || !patch_rings_ok(P.rings))
    return hipErrorInvalidValue;
  int pxc = 0, py0 = 0;
  const unsigned grid = patch_grid(n, m, patch_th(P.rings), line_lo, line_hi, &pxc, &py0);
  if (grid == 0) return hipSuccess;
  const int xm = g_xcd_map ? 1 : 0;  // halo lines of neighbouring patches meet in one L2
  return patch_dispatch(P.un, P.umask, P.nt != 0, [&](auto U, auto M, auto NTF) {
#define AMG_UP(RG)                                                                                            \
  hipLaunchKernelGGL((patch_up_kernel<decltype(U)::value, decltype(M)::value, decltype(NTF)::value, RG>),     \
                     dim3(grid), dim3(PATCH_NT), 0, st, (int)n, (int)m, pxc, P.rtype, P.ptab, P.utabd, P.utabi, \
                     P.nent, P.ntypes, x, f, uH, (int)nH, u_out, omega, xm, py0, P.tflag, P.ctype)
    if (P.rings == 2) AMG_UP(2);
    else AMG_UP(3);
#undef AMG_UP
  });
}
// The seam kernel's frame: 48 held lines x 76 columns [-6, 70), 38 output lines, 456 threads (eight
// waves, the last one of 8 lanes), three workgroups per CU at 6 waves per SIMD (76 registers, 36.5 KB
// of LDS, no scratch).  Timed alone on 4096^2 against the two legs it replaces (217 us): 48 x 76
// 196 us, 40 x 76 (30 lines, four workgroups per CU) 223 us, 56 x 76 (46 lines, 7 waves per SIMD,
// 72 registers) 247 us ("K-Patch seam").
using SeamFrame = PatchFrameT<48, 76>;
constexpr int PATCH_SEAM_WAVES = 6;
int patch_seam_lines() { return SeamFrame::th(PATCH_SEAM_RINGS); }
static bool patch_seam_geometry_ok(int64_t n, int64_t m) {
  return patch_geometry_ok(n, m) && n < ((int64_t)1 << 31) - 64 * m - 128;
}
static_assert(SeamFrame::EC == 76, "patch_frame_columns");
hipError_t launch_patch_seam_flags(int64_t n, int64_t m, const uint8_t* rtype, int ntypes, uint8_t* flag,
                                   int64_t* n_tiles, hipStream_t st, uint8_t* ctype) {
  if (!patch_seam_geometry_ok(n, m)) return hipErrorInvalidValue;
  const int64_t lines = (n + m - 1) / m;
  const int pxc = (int)(m / PATCH_TW);
  const int64_t th = patch_seam_lines();
  const int64_t tiles = (lines + th - 1) / th * pxc;
  if (n_tiles) *n_tiles = tiles;
  if (!flag) return hipSuccess;
  hipLaunchKernelGGL(patch_tile_flags_kernel, dim3((unsigned)tiles), dim3(256), 0, st, (int)n, (int)m, pxc,
                     PATCH_SEAM_RINGS, SeamFrame::EH, SeamFrame::EC, rtype, ntypes, flag,
                     ntypes < (int)PATCH_FLAG_COLTYPED ? ctype : nullptr);
  return hipGetLastError();
}
hipError_t launch_patch_seam(int64_t n, int64_t m, const PatchRef& P, const double* x, const double* f,
                             const double* uH, int64_t nH, double* u_out, double* fH, double omega,
                             hipStream_t st) {
  if (!patch_seam_geometry_ok(n, m) || !P.rtype || !P.ptab || !P.utabd || !P.utabi ||
      (P.ntypes + 1) * patch_un(P.un) > PATCH_MAXTAB || P.nent != P.ntypes * patch_un(P.un) || !x || !f || !uH ||
      nH < 2 || !u_out || u_out == x || !fH || P.rings != PATCH_SEAM_RINGS || patch_un(P.un) != 5)
    return hipErrorInvalidValue;
  int pxc = 0, py0 = 0;
  const unsigned grid = patch_grid(n, m, patch_seam_lines(), 0, -1, &pxc, &py0);
  if (grid == 0) return hipSuccess;
  const int xm = g_xcd_map ? 1 : 0;
  // (the 5-point kind alone is instantiated: a 7- or 9-point level 0 keeps the two launches)
#define AMG_SEAM(NTF)                                                                                          \
  hipLaunchKernelGGL((patch_seam_kernel<5, 0x0BA, NTF, SeamFrame, PATCH_SEAM_WAVES>), dim3(grid), dim3(SeamFrame::NT), \
                     0, st, (int)n, (int)m, pxc, P.rtype, P.ptab, P.utabd, P.utabi, P.nent, P.ntypes, x, f, uH,  \
                     (int)nH, u_out, fH, omega, xm, P.tflag, P.ctype)
  if (P.nt) AMG_SEAM(true);
  else AMG_SEAM(false);
#undef AMG_SEAM
  return hipGetLastError();
}
// the halo a patch is loaded with (3 lines above and below, 4 columns left and right; the lines
// beyond are guard lines of zeros) bounds the dependent stages of one launch: stage s of S reads
// ring S - s, and the residual + restriction take a ring and a column of their own
int patch_rb_max_stages(bool tail) { return tail ? 2 : 3; }
uint32_t patch_rb_stages(const int* colors, int count) {
  uint32_t v = (uint32_t)count & 7u;
  for (int q = 0; q < count && q < 4; ++q) v |= ((uint32_t)colors[q] & 3u) << (4 + 2 * q);
  return v;
}
hipError_t launch_patch_rb(bool prolong, bool tail, int64_t n, int64_t m, const PatchRef& P, const double* x,
                           const double* f, const double* uH, int64_t nH, double* u_out, double* r_out,
                           double* fH, double* uH_zero, uint32_t stages, uint32_t ctab, hipStream_t st,
                           int64_t line_lo, int64_t line_hi) {
  const int nst = (int)(stages & 7u);
  if (!patch_geometry_ok(n, m) || !P.rtype || !P.ptab || !P.utabd || !P.utabi || (P.ntypes + 1) * patch_un(P.un) > PATCH_MAXTAB ||
      P.nent != P.ntypes * patch_un(P.un) || !u_out || u_out == x || (prolong && (!uH || tail)) || (tail && !fH) || nH < 2 ||
      nst < 1 || nst > patch_rb_max_stages(tail) || (m & 1) || P.rings != 3)
    return hipErrorInvalidValue;
  int pxc = 0, py0 = 0;
  const unsigned grid = patch_grid(n, m, patch_th(3), line_lo, line_hi, &pxc, &py0);
  if (grid == 0) return hipSuccess;
  const int xm = g_xcd_map ? 1 : 0;
  return patch_dispatch(P.un, P.umask, P.nt != 0, [&](auto U, auto M, auto NTF) {
#define AMG_RB(PRO, TL)                                                                              \
  hipLaunchKernelGGL((patch_rb_kernel<decltype(U)::value, decltype(M)::value, decltype(NTF)::value, PRO, TL>), dim3(grid), \
                     dim3(PATCH_NT), 0, st, (int)n, (int)m, pxc, P.rtype, P.ptab, P.utabd, P.utabi,    \
                     P.nent, P.ntypes, x, f, uH, (int)nH, u_out, r_out, fH, uH_zero, stages, ctab, xm, py0,  \
                     P.tflag)
    if (tail) AMG_RB(false, true);
    else if (prolong) AMG_RB(true, false);
    else AMG_RB(false, false);
#undef AMG_RB
  });
}
int patch_lds_pitch() { return PATCH_EC; }
int patch_max_entries() { return PATCH_MAXTAB; }

// ---- one colour of the multicolour Gauss-Seidel sweep, dictionary-coded -----------------
// Storage rows [p0, p0 + count) are the rows of one colour (host_setup.hpp: ColorPerm),
// rowid[p] the dof each one updates (-1 = padding); codes are indexed by storage row,
// offsets are relative to the dof.  u is updated in place: rows of one colour do not
// reference each other.  Same arithmetic as K-SELL's CSR_GS mode.
template <int WORDS, int UN>
__global__ __launch_bounds__(256) void dict_gs_color_kernel(
    int p0, int count, const uint64_t* __restrict__ codes, const int32_t* __restrict__ rowid,
    const int32_t* __restrict__ doff, const double* __restrict__ dval, int ntab,
    const double* __restrict__ f, double* u, int xcd_map) {
  typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));
  __shared__ DictEntry tab[256];
  const int k = xcd_tile(blockIdx.x, gridDim.x, xcd_map) * 256 + (int)threadIdx.x;
  const int p = p0 + k;
  const int row = k < count ? rowid[p] : -1;
  DictStream<WORDS, 1> s;
  s.live[0] = row >= 0;
  s.cw[0][0] = s.cw[0][1] = ~(uint64_t)0;
  s.ty = 0xFFFFu;
  s.fi[0] = s.xi[0] = 0.0;
  if (s.live[0]) {
    const uint64_t* cp = codes + (int64_t)p * WORDS;
    if (WORDS == 2) {
      const u64x2 t = *reinterpret_cast<const u64x2*>(cp);
      s.cw[0][0] = t.x; s.cw[0][1] = t.y;
    } else {
      s.cw[0][0] = cp[0];
    }
    s.fi[0] = f[row];
    s.xi[0] = u[row];
  }
  dict_stage_table<CSR_GS>(tab, doff, dval, ntab);
  __syncthreads();
  double res[1];
  dict_rows<CSR_GS, WORDS, UN, 1>(s, s.live[0] ? row : 0, tab, u, 1.0, 0, res);
  if (s.live[0]) u[row] = res[0];
}
// The whole symmetric pass (colours 0 .. nc-1, then nc-1 .. 0) of a SMALL level in one launch:
// one workgroup, a barrier between colours (__syncthreads also orders the global accesses of
// the workgroup).  On the launch-bound levels of a deep hierarchy a pass is 2 nc launches of
// ~4.6 us each with almost nothing to do; here it is 2 nc barriers.  Same rows, same order of
// the colours, same row arithmetic: same bits.
template <int WORDS, int UN>
__global__ __launch_bounds__(1024) void dict_gs_sweep_kernel(
    int nc, const int32_t* __restrict__ starts, const uint64_t* __restrict__ codes,
    const int32_t* __restrict__ rowid, const int32_t* __restrict__ doff,
    const double* __restrict__ dval, int ntab, const double* __restrict__ f, double* u) {
  typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));
  __shared__ DictEntry tab[256];
  if (threadIdx.x < 256) dict_stage_table<CSR_GS>(tab, doff, dval, ntab);
  __syncthreads();
  for (int phase = 0; phase < 2 * nc; ++phase) {
    const int c = phase < nc ? phase : 2 * nc - 1 - phase;
    const int p0 = starts[c], count = starts[c + 1] - p0;
    for (int k = threadIdx.x; k < count; k += 1024) {
      const int p = p0 + k;
      const int row = rowid[p];
      DictStream<WORDS, 1> s;
      s.live[0] = row >= 0;
      s.cw[0][0] = s.cw[0][1] = ~(uint64_t)0;
      s.ty = 0xFFFFu;
      s.fi[0] = s.xi[0] = 0.0;
      if (s.live[0]) {
        const uint64_t* cp = codes + (int64_t)p * WORDS;
        if (WORDS == 2) {
          const u64x2 t = *reinterpret_cast<const u64x2*>(cp);
          s.cw[0][0] = t.x; s.cw[0][1] = t.y;
        } else {
          s.cw[0][0] = cp[0];
        }
        s.fi[0] = f[row];
        s.xi[0] = u[row];
      }
      double res[1];
      dict_rows<CSR_GS, WORDS, UN, 1>(s, s.live[0] ? row : 0, tab, u, 1.0, 0, res);
      if (s.live[0]) u[row] = res[0];
    }
    __syncthreads();  // colour c is complete (and visible) before the next one reads it
  }
}
hipError_t launch_dict_gs_sweep(int nc, const int32_t* starts_dev, int64_t n_storage, int words, int wmax,
                                const uint64_t* codes, const int32_t* rowid, const int32_t* doff,
                                const double* dval, int ntab, const double* f, double* u,
                                hipStream_t st) {
  if (nc <= 0) return hipSuccess;
  if (!starts_dev || n_storage >= ((int64_t)1 << 31) - 512 || ntab > 255 || (words != 1 && words != 2) ||
      wmax > 8 * words)
    return hipErrorInvalidValue;
#define AMG_DICT_GSS(W, U)                                                                   \
  hipLaunchKernelGGL((dict_gs_sweep_kernel<W, U>), dim3(1), dim3(1024), 0, st, nc, starts_dev, \
                     codes, rowid, doff, dval, ntab, f, u)
  if (words == 1) {
    if (wmax <= 3) AMG_DICT_GSS(1, 3);
    else if (wmax <= 5) AMG_DICT_GSS(1, 5);
    else if (wmax <= 7) AMG_DICT_GSS(1, 7);
    else AMG_DICT_GSS(1, 8);
  } else {
    if (wmax <= 9) AMG_DICT_GSS(2, 9);
    else if (wmax <= 12) AMG_DICT_GSS(2, 12);
    else AMG_DICT_GSS(2, 16);
  }
#undef AMG_DICT_GSS
  return hipGetLastError();
}
hipError_t launch_dict_gs_color(int64_t p0, int64_t count, int words, int wmax,
                                const uint64_t* codes, const int32_t* rowid, const int32_t* doff,
                                const double* dval, int ntab, const double* f, double* u,
                                hipStream_t st) {
  if (count <= 0) return hipSuccess;
  if (p0 + count >= ((int64_t)1 << 31) - 512 || ntab > 255 || (words != 1 && words != 2) ||
      wmax > 8 * words)
    return hipErrorInvalidValue;
  const unsigned grid = (unsigned)((count + 255) / 256);
#define AMG_DICT_GS(W, U)                                                                       \
  hipLaunchKernelGGL((dict_gs_color_kernel<W, U>), dim3(grid), dim3(256), 0, st, (int)p0,        \
                     (int)count, codes, rowid, doff, dval, ntab, f, u, g_xcd_map)
  if (words == 1) {
    if (wmax <= 3) AMG_DICT_GS(1, 3);
    else if (wmax <= 5) AMG_DICT_GS(1, 5);
    else if (wmax <= 7) AMG_DICT_GS(1, 7);
    else AMG_DICT_GS(1, 8);
  } else {
    if (wmax <= 9) AMG_DICT_GS(2, 9);
    else if (wmax <= 12) AMG_DICT_GS(2, 12);
    else AMG_DICT_GS(2, 16);
  }
#undef AMG_DICT_GS
  return hipGetLastError();
}

// (W, U) dispatch shared by the fused launchers: F is a generic lambda taking
// std::integral_constant<int, W>, <int, U>, <bool, NT>, <int, R>
template <class F>
static hipError_t dict_dispatch(int words, int wmax, bool nt, bool two, F&& go) {
  using std::integral_constant;
  auto with_nr = [&](auto W, auto U) -> hipError_t {
    if (two) {
      if (nt) go(W, U, integral_constant<bool, true>{}, integral_constant<int, 2>{});
      else go(W, U, integral_constant<bool, false>{}, integral_constant<int, 2>{});
    } else {
      if (nt) go(W, U, integral_constant<bool, true>{}, integral_constant<int, 1>{});
      else go(W, U, integral_constant<bool, false>{}, integral_constant<int, 1>{});
    }
    return hipGetLastError();
  };
  if (words == 1) {
    if (wmax <= 3) return with_nr(integral_constant<int, 1>{}, integral_constant<int, 3>{});
    if (wmax <= 5) return with_nr(integral_constant<int, 1>{}, integral_constant<int, 5>{});
    if (wmax <= 7) return with_nr(integral_constant<int, 1>{}, integral_constant<int, 7>{});
    return with_nr(integral_constant<int, 1>{}, integral_constant<int, 8>{});
  }
  if (wmax <= 9) return with_nr(integral_constant<int, 2>{}, integral_constant<int, 9>{});
  if (wmax <= 12) return with_nr(integral_constant<int, 2>{}, integral_constant<int, 12>{});
  return with_nr(integral_constant<int, 2>{}, integral_constant<int, 16>{});
}
static bool dict_args_ok(int64_t n, int words, int wmax, int ntab) {
  return n < ((int64_t)1 << 31) - 1024 && ntab <= 255 && (words == 1 || words == 2) &&
         wmax <= 8 * words;
}
static bool aligned16(const void* a, const void* b, const void* c) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) |
           reinterpret_cast<uintptr_t>(c)) & 15) == 0;
}
// The contiguous-run-per-XCD tile order pays where the level lives in the caches (levels
// 2+ of the 4096^2 hierarchy: -1..3 us per launch); on the streamed levels beyond the
// Infinity Cache the plain order is faster (level 0: 91 vs 94 us per sweep, fused
// residual 108 vs 114 us), although it fetches x 2x at the L2 -- measured per level.
// tile_rows: rows a workgroup advances by.  A band of >= 16 tiles (the 3-D levels) takes the
// slab-per-plane order whatever the size of the level (xcd_tile).
static int g_xcd_slab = 1;
// paired-load path of wave-uniform 7- / 15-point rows (set_dict_stencil / AMG_HIP_DICT_STENCIL=0: A/B switch)
static int g_dict_stencil = [] {
  const char* e = std::getenv("AMG_HIP_DICT_STENCIL");
  return (e && *e == '0') ? 0 : 1;
}();
static const double* dict_stencil_tab(const DictRef& D, const double* x) {
  return (g_dict_stencil && D.utd && D.uti && D.rtype && (reinterpret_cast<uintptr_t>(x) & 15) == 0) ? D.utd : nullptr;
}
static int dict_xcd_map(const DictRef& D, int64_t tile_rows = 512) {
  if (!g_xcd_map) return 0;
  const int64_t tp = D.hb / tile_rows / 8 * 8;
  if (g_xcd_slab && tp >= 16 && tp <= (1 << 20)) return (int)tp;
  return D.nt ? 0 : 1;
}
// two rows per lane need 16-byte aligned f / out / codes (vector lane accesses)
static bool dict_two_rows(int64_t n, const DictRef& D, const void* f, const void* out) {
  return g_dict_rows_per_lane == 2 && n >= 4096 && aligned16(f, out, D.rtype ? nullptr : D.codes) &&
         (!D.rtype || (reinterpret_cast<uintptr_t>(D.rtype) & 1) == 0);
}
hipError_t launch_dict_resid_restrict(int64_t n, const DictRef& D, const double* x,
                                      const double* f, double* r_out, int64_t nH, double* fH,
                                      const double* diagH, double* uH1, double* uH0,
                                      double omega, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (!dict_args_ok(n, D.words, D.wmax, D.ntab) || nH > n || !fH || (uH1 ? !diagH : !uH0))
    return hipErrorInvalidValue;
  const bool two = dict_two_rows(n, D, f, r_out);  // r_out may be nullptr (not stored)
  const int64_t stride = 256 * (two ? 2 : 1) - 2;
  const unsigned tiles = (unsigned)((n + stride - 1) / stride);
  return dict_dispatch(D.words, D.wmax, D.nt != 0, two, [&](auto W, auto U, auto NTF, auto RR) {
    hipLaunchKernelGGL((dict_resid_restrict_kernel<decltype(W)::value, decltype(U)::value,
                                                   decltype(NTF)::value, decltype(RR)::value>),
                       dim3(tiles), dim3(256), 0, st, (int)n, D.codes, D.rtype, D.rwords, D.doff,
                       D.dval, D.ntab, x, f, r_out, (int)nH, fH, diagH, uH1, uH0, omega, dict_xcd_map(D, stride),
                       dict_stencil_tab(D, x), D.uti);
  });
}
hipError_t launch_dict_jacobi_prolong(int64_t n, const DictRef& D, const double* x,
                                      const double* f, double* out, double omega, int64_t n_h,
                                      const double* uh_in, double* uh_out, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (!dict_args_ok(n_h, D.words, D.wmax, D.ntab) || n > n_h || !uh_in || !uh_out ||
      ((reinterpret_cast<uintptr_t>(uh_in) | reinterpret_cast<uintptr_t>(uh_out)) & 15) != 0)
    return hipErrorInvalidValue;
  const bool two = dict_two_rows(n, D, f, out);
  const int64_t stride = 256 * (two ? 2 : 1) - 2;
  const unsigned tiles = (unsigned)((n + stride - 1) / stride);
  return dict_dispatch(D.words, D.wmax, D.nt != 0, two, [&](auto W, auto U, auto NTF, auto RR) {
    hipLaunchKernelGGL((dict_jacobi_prolong_kernel<decltype(W)::value, decltype(U)::value,
                                                   decltype(NTF)::value, decltype(RR)::value>),
                       dim3(tiles), dim3(256), 0, st, (int)n, D.codes, D.rtype, D.rwords, D.doff,
                       D.dval, D.ntab, x, f, out, omega, (int)n_h, uh_in, uh_out, dict_xcd_map(D, stride),
                       dict_stencil_tab(D, x), D.uti);
  });
}
// the two-sweep forms for small levels; see dict_pair_down_kernel / dict_pair_up_kernel
bool dict_pair_ok(int64_t n, const DictRef& D, int hb, const void* a, const void* b, const void* c) {
  return hb >= 0 && hb <= PAIR_HB - 1 && n >= 256 && n <= 400000 && !D.nt &&
         dict_args_ok(n, D.words, D.wmax, D.ntab) && g_dict_rows_per_lane == 2 &&
         aligned16(a, b, c) && aligned16(D.rtype ? nullptr : D.codes, nullptr, nullptr) &&
         (!D.rtype || (reinterpret_cast<uintptr_t>(D.rtype) & 1) == 0);
}
// The (WORDS, UN) a level's rows are walked with, as a class 0 .. 6: one table for the pair kernels
// and for the K-Duo kernels, which take one class per level.
template <int C> struct DictWU;
template <> struct DictWU<0> { static constexpr int W = 1, U = 3; };
template <> struct DictWU<1> { static constexpr int W = 1, U = 5; };
template <> struct DictWU<2> { static constexpr int W = 1, U = 7; };
template <> struct DictWU<3> { static constexpr int W = 1, U = 8; };
template <> struct DictWU<4> { static constexpr int W = 2, U = 9; };
template <> struct DictWU<5> { static constexpr int W = 2, U = 12; };
template <> struct DictWU<6> { static constexpr int W = 2, U = 16; };
constexpr int DICT_WU_CLASSES = 7;
static int dict_wu_class(int words, int wmax) {
  if (words == 1) return wmax <= 3 ? 0 : (wmax <= 5 ? 1 : (wmax <= 7 ? 2 : 3));
  return wmax <= 9 ? 4 : (wmax <= 12 ? 5 : 6);
}
template <int C, class F>
static void dict_dispatch_class(int c, F&& go) {
  if constexpr (C < DICT_WU_CLASSES) {
    if (c == C) go(std::integral_constant<int, DictWU<C>::W>{}, std::integral_constant<int, DictWU<C>::U>{});
    else dict_dispatch_class<C + 1>(c, go);
  }
}
template <class F>
static hipError_t dict_dispatch_wu(int words, int wmax, F&& go) {
  dict_dispatch_class<0>(dict_wu_class(words, wmax), go);
  return hipGetLastError();
}
hipError_t launch_dict_pair_down(int64_t n, const DictRef& D, int hb, const double* a,
                                 const double* f, double* u_out, double* r_out, int64_t nH,
                                 double* fH, const double* diagH, double* uH1, double omega,
                                 hipStream_t st) {
  if (!dict_pair_ok(n, D, hb, a, f, u_out) || !fH || !diagH || !uH1 || nH > n ||
      (r_out && (reinterpret_cast<uintptr_t>(r_out) & 15)))
    return hipErrorInvalidValue;
  const int hbw = (hb + 1) & ~1;
  const unsigned tiles = (unsigned)((n + 509) / 510);
  return dict_dispatch_wu(D.words, D.wmax, [&](auto W, auto U) {
    hipLaunchKernelGGL((dict_pair_down_kernel<decltype(W)::value, decltype(U)::value>), dim3(tiles),
                       dim3(256), 0, st, (int)n, D.codes, D.rtype, D.rwords, D.doff, D.dval, D.ntab,
                       a, f, u_out, r_out, (int)nH, fH, diagH, uH1, omega, hbw, dict_xcd_map(D));
  });
}
hipError_t launch_dict_pair_up(int64_t n, const DictRef& D, int hb, const double* a,
                               const double* f, double* u_out, double omega, int64_t n_h,
                               const double* uh_in, double* uh_out, hipStream_t st) {
  if (!dict_pair_ok(n, D, hb, a, f, u_out) || n > n_h || !uh_in || !uh_out ||
      ((reinterpret_cast<uintptr_t>(uh_in) | reinterpret_cast<uintptr_t>(uh_out)) & 15) != 0)
    return hipErrorInvalidValue;
  const int hbw = (hb + 1) & ~1;
  const unsigned tiles = (unsigned)((n + 509) / 510);
  return dict_dispatch_wu(D.words, D.wmax, [&](auto W, auto U) {
    hipLaunchKernelGGL((dict_pair_up_kernel<decltype(W)::value, decltype(U)::value>), dim3(tiles),
                       dim3(256), 0, st, (int)n, D.codes, D.rtype, D.rwords, D.doff, D.dval, D.ntab,
                       a, f, u_out, omega, hbw, (int)n_h, uh_in, uh_out, dict_xcd_map(D));
  });
}
// K-Duo (dict_duo_down_kernel / dict_duo_up_kernel).  The windows of both legs, for the launchers, the
// host's predicate and the tests: 0 when every window is within its capacity.
int duo_windows_host(int hb0, int hb1, int tile_rows, int32_t* out) {
  if (hb0 < 0 || hb1 < 0 || hb0 > PAIR_HB - 1 || hb1 > PAIR_HB - 1 || tile_rows < 4 || (tile_rows & 1) ||
      tile_rows > DUO_T || !out)
    return 1;
  int w[DW_COUNT];
  duo_windows((hb0 + 1) & ~1, (hb1 + 1) & ~1, tile_rows, w);
  for (int i = 0; i < DW_COUNT; ++i) out[i] = w[i];
  return (w[DW_D_M1] <= DUO_D_M1 && w[DW_D_M0] <= DUO_D_M0 && w[DW_D_A0] <= DUO_D_A0 && w[DW_U_M1] <= DUO_U_M1 &&
          w[DW_U_A1] <= DUO_U_A1 && w[DW_U_M0] <= DUO_U_M0 && w[DW_U_A0] <= DUO_U_A0)
             ? 0
             : 1;
}
int duo_owned_host(int tile, int tile_rows, int32_t* out) {
  if (tile < 0 || tile_rows < 4 || (tile_rows & 1) || tile_rows > DUO_T || !out ||
      (int64_t)tile * tile_rows > ((int64_t)1 << 30))
    return 1;
  int o[6];
  duo_owned(tile * tile_rows, tile_rows, o);
  for (int i = 0; i < 6; ++i) out[i] = o[i];
  return 0;
}
// (WORDS, UN) of a level as dict_dispatch_wu picks it, as a class 0 .. 6; the duo kernels exist for a
// coarser level of the same class as the finer one, of up to DUO_CLASS_SPAN classes below it (the rows
// of a Galerkin hierarchy get shorter as the band narrows: 4096^2 pairs <2,9>/<2,9>, <2,9>/<1,7> and
// <1,5>/<1,5>) or of the class above (the level under a 5-point fine level: 8 entries over 9).  Any
// other pair of levels keeps the pair form.
constexpr int DUO_CLASS_SPAN = 3;
static int duo_class(const DictRef& D) { return dict_wu_class(D.words, D.wmax); }
template <int C0, int K, class F>
static bool duo_dispatch_c1(int c1, F&& go) {
  if constexpr (K > DUO_CLASS_SPAN) {
    return false;
  } else if constexpr (C0 - K < 0 || C0 - K >= DICT_WU_CLASSES) {
    return duo_dispatch_c1<C0, K + 1>(c1, go);
  } else {
    if (c1 == C0 - K) {
      go(std::integral_constant<int, C0>{}, std::integral_constant<int, C0 - K>{});
      return true;
    }
    return duo_dispatch_c1<C0, K + 1>(c1, go);
  }
}
template <int C0, class F>
static bool duo_dispatch_c0(int c0, int c1, F&& go) {
  if constexpr (C0 < DICT_WU_CLASSES) {
    if (c0 == C0) return duo_dispatch_c1<C0, -1>(c1, go);
    return duo_dispatch_c0<C0 + 1>(c0, c1, go);
  } else {
    return false;
  }
}
// DUO_MAX_ROWS: a finer level with more rows runs its two pair launches.  Above it a level is bound by
// its rows, not by its launches, and the recomputed halo costs more than the launch saves (DESIGN.md
// section 4, K-Duo; 4096^2 hierarchy, down + up leg of the duo against the four pair launches: level 6,
// 262 144 rows, 19.4 + 17.4 us against 15.6 + 15.5 us; level 7, 131 072 rows, 15.7 + 14.4 us against
// 12.4 + 12.8 us; level 8, 65 536 rows, 10.0 + 9.9 us against 11.5 + 11.3 us)
constexpr int64_t DUO_MAX_ROWS = 100000;
int duo_tile_rows(int hb0) { return ((hb0 + 1) & ~1) <= DUO_T_SMALL_HBW ? DUO_T_SMALL : DUO_T; }
bool dict_duo_ok(int64_t n0, const DictRef& D0, int hb0, int64_t n1, const DictRef& D1, int hb1, int64_t n2) {
  int32_t w[DW_COUNT];
  const int c0 = duo_class(D0), c1 = duo_class(D1);
  return n0 <= DUO_MAX_ROWS && n1 >= 1 && n2 >= 1 && n1 <= (n0 + 1) / 2 && n2 <= (n1 + 1) / 2 &&
         dict_pair_ok(n0, D0, hb0, nullptr, nullptr, nullptr) && dict_pair_ok(n1, D1, hb1, nullptr, nullptr, nullptr) &&
         c1 <= c0 + 1 && c0 - c1 <= DUO_CLASS_SPAN && duo_windows_host(hb0, hb1, duo_tile_rows(hb0), w) == 0;
}
hipError_t launch_dict_duo_down(int64_t n0, const DictRef& D0, int hb0, int64_t n1, const DictRef& D1, int hb1,
                                const double* a0, const double* f0, double* u0_out, double* r0_out,
                                double* f1_out, const double* diag1, double* u1_out, double* r1_out, int64_t n2,
                                double* f2_out, const double* diag2, double* v2_out, double omega,
                                hipStream_t st) {
  if (!dict_duo_ok(n0, D0, hb0, n1, D1, hb1, n2) || !a0 || !f0 || !u0_out || !f1_out || !diag1 || !u1_out ||
      !f2_out || !diag2 || !v2_out || !aligned16(a0, f0, diag1) || !aligned16(r0_out, nullptr, nullptr))
    return hipErrorInvalidValue;
  const int hbw0 = (hb0 + 1) & ~1, hbw1 = (hb1 + 1) & ~1;
  const int T = duo_tile_rows(hb0);
  const unsigned tiles = (unsigned)((n0 + T - 1) / T);
  const bool found = duo_dispatch_c0<0>(duo_class(D0), duo_class(D1), [&](auto C0, auto C1) {
    using K0 = DictWU<decltype(C0)::value>;
    using K1 = DictWU<decltype(C1)::value>;
    hipLaunchKernelGGL((dict_duo_down_kernel<K0::W, K0::U, K1::W, K1::U>), dim3(tiles), dim3(256), 0, st, (int)n0,
                       D0.codes, D0.rtype, D0.rwords, D0.doff, D0.dval, D0.ntab, hbw0, (int)n1, D1.codes, D1.rtype,
                       D1.rwords, D1.doff, D1.dval, D1.ntab, hbw1, a0, f0, u0_out, r0_out, f1_out, diag1, u1_out,
                       r1_out, (int)n2, f2_out, diag2, v2_out, omega, T, dict_xcd_map(D0));
  });
  return found ? hipGetLastError() : hipErrorInvalidValue;
}
hipError_t launch_dict_duo_up(int64_t n0, const DictRef& D0, int hb0, int64_t n1, const DictRef& D1, int hb1,
                              const double* a1, const double* f1, double* u1_out, const double* u0_in,
                              const double* f0, double* u0_out, double omega, int64_t n_h, const double* uh_in,
                              double* uh_out, hipStream_t st) {
  if (!dict_duo_ok(n0, D0, hb0, n1, D1, hb1, 1) || !a1 || !f1 || !u1_out || !u0_in || !f0 || !u0_out ||
      u0_out == u0_in || n0 > n_h || !uh_in || !uh_out || !aligned16(a1, f1, u0_in) || !aligned16(f0, u0_out, uh_in) ||
      !aligned16(uh_out, nullptr, nullptr))
    return hipErrorInvalidValue;
  const int hbw0 = (hb0 + 1) & ~1, hbw1 = (hb1 + 1) & ~1;
  const int T = duo_tile_rows(hb0);
  const unsigned tiles = (unsigned)((n0 + T - 1) / T);
  const bool found = duo_dispatch_c0<0>(duo_class(D0), duo_class(D1), [&](auto C0, auto C1) {
    using K0 = DictWU<decltype(C0)::value>;
    using K1 = DictWU<decltype(C1)::value>;
    hipLaunchKernelGGL((dict_duo_up_kernel<K0::W, K0::U, K1::W, K1::U>), dim3(tiles), dim3(256), 0, st, (int)n0,
                       D0.codes, D0.rtype, D0.rwords, D0.doff, D0.dval, D0.ntab, hbw0, (int)n1, D1.codes, D1.rtype,
                       D1.rwords, D1.doff, D1.dval, D1.ntab, hbw1, a1, f1, u1_out, u0_in, f0, u0_out, omega,
                       (int)n_h, uh_in, uh_out, T, dict_xcd_map(D0));
  });
  return found ? hipGetLastError() : hipErrorInvalidValue;
}
// ---- K-March: two true-Jacobi sweeps of a 3-D 7-point level in ONE pass ---------------------
// On the finest level of a 3-D hierarchy a sweep streams x, f and the output again (25 B per row),
// and the +-plane neighbours defeat the 2-D patch form (three rings around planes x lines x columns
// leave a quarter of a patch as output).  Here a workgroup owns a tile of TL lines x TC columns and
// MARCHES through the planes: x of plane q arrives (tile + 2 rings in the plane), the first sweep is
// formed on plane q-1 (tile + 1 ring) from the x planes q-2, q-1, q, the second sweep on plane q-2
// (tile) from the first-sweep planes q-3, q-2, q-1 -- two rings of three planes in LDS, two barriers
// per plane, only the two in-plane directions pay a halo.  Row structure from the row TYPE: the
// values of every type laid out by pattern position {-M, -m, -1, (0), +1, +m, +M} by the host
// (positions a boundary row does not have: +0.0, its diagonal apart); waves of interior cells take
// the interior type's values from kernel arguments.  Same products in the same (ascending column)
// order, the same IEEE division and relaxation expression as dict_rows<CSR_JACOBI>, adding (+0.0) x
// where dict_rows adds it for absent slots -> same bits as two launches of the sweep.
constexpr int MARCH_TL = 16, MARCH_TC = 64, MARCH_NT = 512;  // (8 lines x 256 threads: 0.8 % slower)
constexpr int MARCH_XL = MARCH_TL + 4, MARCH_XC = MARCH_TC + 4;  // x tile: 20 x 68
constexpr int MARCH_SL = MARCH_TL + 2, MARCH_SC = MARCH_TC + 2;  // first-sweep tile: 18 x 66
constexpr int MARCH_XN = MARCH_XL * MARCH_XC, MARCH_SN = MARCH_SL * MARCH_SC;
constexpr int MARCH_XS = (MARCH_XN + MARCH_NT - 1) / MARCH_NT;   // x cells per thread (3)
constexpr int MARCH_SS = (MARCH_SN + MARCH_NT - 1) / MARCH_NT;   // first-sweep cells per thread (3)
constexpr int MARCH_OS = MARCH_TL * MARCH_TC / MARCH_NT;         // output cells per thread (2)
constexpr int MARCH_TYPES = 64;
typedef MarchRef MarchArgs;
// one Jacobi update of a cell from its six neighbours nb[] (-M, -m, -1, +1, +m, +M) and itself
__device__ __forceinline__ double march_update(const double (&w)[6], double diag, const double (&nb)[6],
                                               double xi, double fi, double omega) {
  double acc = 0.0;
#pragma unroll
  for (int u = 0; u < 6; ++u) acc += w[u] * nb[u];
  const bool nod = diag == 0.0;
  const double q = (fi - acc) / (nod ? 1.0 : diag);  // smoother.hpp:136
  return nod ? xi : xi + omega * (q - xi);
}
__global__ __launch_bounds__(MARCH_NT) void march_kernel(MarchArgs A) {
  __shared__ double X[3][MARCH_XN];
  __shared__ double S[3][MARCH_SN];
  __shared__ double wt[MARCH_TYPES * 8];  // per type: w[6] (pattern order without the diagonal), diagonal, -
  const int tid = (int)threadIdx.x;
  const int tiles_c = A.m / MARCH_TC, tiles_l = A.lines / MARCH_TL;
  const int tile = (int)blockIdx.x % (tiles_c * tiles_l), chunk = (int)blockIdx.x / (tiles_c * tiles_l);
  const int l0 = (tile / tiles_c) * MARCH_TL, c0 = (tile % tiles_c) * MARCH_TC;
  const int pa = chunk * A.chunk_planes, pb = min(pa + A.chunk_planes, A.planes);
  for (int q = tid; q < A.ntypes * 8; q += MARCH_NT) wt[q] = A.wtab[q];
  // cells of this thread
  int xoff[MARCH_XS];   // global row offset inside a plane (line * m + col), or -1 outside the domain
#pragma unroll
  for (int k = 0; k < MARCH_XS; ++k) {
    const int q = k * MARCH_NT + tid;
    const int line = l0 - 2 + q / MARCH_XC, col = c0 - 2 + q % MARCH_XC;
    xoff[k] = (q < MARCH_XN && line >= 0 && line < A.lines && col >= 0 && col < A.m) ? line * A.m + col : -1;
  }
  // first-sweep cells of this thread: its two OUTPUT cells (so that their f and row type are still in
  // registers when the second sweep reaches the plane, one step later) and one cell of the ring
  // around the tile (164 cells: the first 164 threads).  soff: row offset in the plane or -1, si / sx:
  // index in the first-sweep tile / in the x tile.
  static_assert(MARCH_SS == MARCH_OS + 1 && 2 * MARCH_SC + 2 * MARCH_TL <= MARCH_NT, "first-sweep cell map");
  int soff[MARCH_SS], si[MARCH_SS], sx[MARCH_SS];
  int ooff[MARCH_OS];
#pragma unroll
  for (int k = 0; k < MARCH_OS; ++k) {
    const int q = k * MARCH_NT + tid;
    const int ol = q / MARCH_TC, oc = q % MARCH_TC;
    ooff[k] = (l0 + ol) * A.m + c0 + oc;   // always inside the domain
    soff[k] = ooff[k];
    si[k] = (ol + 1) * MARCH_SC + oc + 1;
    sx[k] = (ol + 2) * MARCH_XC + oc + 2;
  }
  {
    const int r = tid;
    int sl, sc;
    if (r < MARCH_SC) { sl = 0; sc = r; }
    else if (r < 2 * MARCH_SC) { sl = MARCH_SL - 1; sc = r - MARCH_SC; }
    else if (r < 2 * MARCH_SC + MARCH_TL) { sl = r - 2 * MARCH_SC + 1; sc = 0; }
    else { sl = r - 2 * MARCH_SC - MARCH_TL + 1; sc = MARCH_SC - 1; }
    const bool ring = r < 2 * MARCH_SC + 2 * MARCH_TL;
    if (!ring) { sl = 1; sc = 1; }
    const int line = l0 - 1 + sl, col = c0 - 1 + sc;
    soff[MARCH_OS] = (ring && line >= 0 && line < A.lines && col >= 0 && col < A.m) ? line * A.m + col : -1;
    si[MARCH_OS] = ring ? sl * MARCH_SC + sc : -1;   // -1: no cell (nothing is stored)
    sx[MARCH_OS] = (sl + 1) * MARCH_XC + sc + 1;
  }
  const int64_t M = (int64_t)A.m * A.lines;
  double xr[MARCH_XS];  // x of the plane that arrives next
  auto fetch_x = [&](int plane) {
#pragma unroll
    for (int k = 0; k < MARCH_XS; ++k)
      xr[k] = (plane >= 0 && plane < A.planes && xoff[k] >= 0) ? A.x[(int64_t)plane * M + xoff[k]] : 0.0;
  };
  double wi[6];
#pragma unroll
  for (int u = 0; u < 6; ++u) wi[u] = A.wint[u];
  const double di = A.dint;
  const uint32_t ti = (uint32_t)A.tint;
  // operands (f, row type) of the first sweep on plane q - 1 and of the second on plane q - 2:
  // requested one plane step ahead, like x (a step is two barriers and a few dozen LDS reads; a
  // global round trip inside it would be most of its time)
  double nf1[MARCH_SS];
  uint32_t nt1[MARCH_SS];
  auto fetch_ops = [&](int q) {
    const int p1 = q - 1;
    const bool live1 = p1 >= pa - 1 && p1 <= pb && p1 >= 0 && p1 < A.planes;
#pragma unroll
    for (int k = 0; k < MARCH_SS; ++k) {
      const bool live = live1 && soff[k] >= 0;
      const int64_t r = live ? (int64_t)p1 * M + soff[k] : 0;
      nf1[k] = live ? A.f[r] : 0.0;
      nt1[k] = live ? (uint32_t)A.rtype[r] : 255u;
    }
  };
  double f2[MARCH_OS];   // operands of the second sweep: what the first sweep used one step ago
  uint32_t t2[MARCH_OS];
#pragma unroll
  for (int k = 0; k < MARCH_OS; ++k) {
    f2[k] = 0.0;
    t2[k] = 255u;
  }
  fetch_x(pa - 2);
  fetch_ops(pa - 2);
  __syncthreads();
  for (int q = pa - 2; q <= pb + 1; ++q) {
    // x of plane q into its ring slot; the next plane is requested
    {
      double* Xq = X[(q + 3) % 3];
#pragma unroll
      for (int k = 0; k < MARCH_XS; ++k)
        if (k * MARCH_NT + tid < MARCH_XN) Xq[k * MARCH_NT + tid] = xr[k];
    }
    const int p1 = q - 1, p2 = q - 2;
    const bool do1 = p1 >= pa - 1 && p1 <= pb;
    const bool do2 = p2 >= pa && p2 < pb;
    double f1[MARCH_SS];
    uint32_t t1[MARCH_SS];
#pragma unroll
    for (int k = 0; k < MARCH_SS; ++k) {
      f1[k] = nf1[k];
      t1[k] = nt1[k];
    }
    fetch_x(q + 1);
    fetch_ops(q + 1);
    lds_barrier();
    if (do1) {  // first sweep on plane q - 1 from the x planes q - 2, q - 1, q
      const double* Xm = X[(q + 1) % 3];  // plane q - 2
      const double* Xc = X[(q + 2) % 3];  // plane q - 1
      const double* Xp = X[(q + 3) % 3];  // plane q
      double* Sq = S[(p1 + 3) % 3];
#pragma unroll
      for (int k = 0; k < MARCH_SS; ++k) {
        const int i = sx[k];
        const double nb[6] = {Xm[i], Xc[i - MARCH_XC], Xc[i - 1], Xc[i + 1], Xc[i + MARCH_XC], Xp[i]};
        const double xi = Xc[i];
        const bool live = t1[k] != 255u;
        double r;
        if (__builtin_amdgcn_ballot_w64(live && t1[k] != ti) == 0) {  // interior (or dead) cells only
          r = march_update(wi, di, nb, xi, f1[k], A.omega);
        } else {
          const uint32_t tt = t1[k] < (uint32_t)MARCH_TYPES ? t1[k] : 0u;
          double w[6];
#pragma unroll
          for (int u = 0; u < 6; ++u) w[u] = wt[tt * 8 + u];
          r = march_update(w, wt[tt * 8 + 6], nb, xi, f1[k], A.omega);
        }
        if (si[k] >= 0) Sq[si[k]] = live ? r : 0.0;
      }
    }
    lds_barrier();
    if (do2) {  // second sweep on plane q - 2 from the first-sweep planes q - 3, q - 2, q - 1
      const double* Sm = S[(p2 + 2) % 3];
      const double* Sc = S[(p2 + 3) % 3];
      const double* Sp = S[(p2 + 4) % 3];
#pragma unroll
      for (int k = 0; k < MARCH_OS; ++k) {
        const int i = si[k];
        const double nb[6] = {Sm[i], Sc[i - MARCH_SC], Sc[i - 1], Sc[i + 1], Sc[i + MARCH_SC], Sp[i]};
        const double xi = Sc[i];
        double r;
        if (__builtin_amdgcn_ballot_w64(t2[k] != ti) == 0) {
          r = march_update(wi, di, nb, xi, f2[k], A.omega);
        } else {
          const uint32_t tt = t2[k] < (uint32_t)MARCH_TYPES ? t2[k] : 0u;
          double w[6];
#pragma unroll
          for (int u = 0; u < 6; ++u) w[u] = wt[tt * 8 + u];
          r = march_update(w, wt[tt * 8 + 6], nb, xi, f2[k], A.omega);
        }
        A.out[(int64_t)p2 * M + ooff[k]] = r;
      }
    }
#pragma unroll
    for (int k = 0; k < MARCH_OS; ++k) {  // plane q - 1 is the second sweep's plane of the next step
      f2[k] = f1[k];
      t2[k] = t1[k];
    }
  }
}
bool march_ok(const MarchRef& A) {
  return A.m >= MARCH_TC && A.m % MARCH_TC == 0 && A.lines >= MARCH_TL && A.lines % MARCH_TL == 0 && A.planes >= 3 &&
         (int64_t)A.m * A.lines * A.planes < ((int64_t)1 << 31) - 1024 && A.ntypes >= 1 && A.ntypes <= MARCH_TYPES &&
         A.tint >= 0 && A.tint < A.ntypes && A.chunk_planes >= 1 && A.wtab && A.rtype && A.x && A.f && A.out &&
         A.out != A.x;
}
hipError_t launch_march(MarchRef A, hipStream_t st) {
  // one wave of workgroups (2 per CU x 256 CUs): as many plane chunks as that takes
  const int64_t tiles = (int64_t)(A.m / MARCH_TC) * (A.lines / MARCH_TL);
  int chunks = (int)std::max<int64_t>(1, std::min<int64_t>(A.planes / 8, (512 + tiles - 1) / tiles));
  A.chunk_planes = (A.planes + chunks - 1) / chunks;
  chunks = (A.planes + A.chunk_planes - 1) / A.chunk_planes;
  if (!march_ok(A)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(march_kernel, dim3((unsigned)(tiles * chunks)), dim3(MARCH_NT), 0, st, A);
  return hipGetLastError();
}
// Setup: does the row-type map describe an m x lines x planes box?  The march loads every cell
// outside [0, m) x [0, lines) as 0, so a row on a column-0 / column-(m-1) / line-0 / line-(lines-1)
// position must not hold the coupling that leaves its line or plane (bits 1 / 2 / 4 / 8 of
// forbid[type]: it holds -1 / +1 / -m / +m); an empty row (type 255) is not a march row either.
__global__ __launch_bounds__(256) void march_box_check_kernel(int64_t n, int m, int lines, MarchForbid F,
                                                              const uint8_t* __restrict__ rtype,
                                                              int32_t* __restrict__ bad) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const uint32_t t = rtype[r];
  const int i = (int)(r % m), j = (int)((r / m) % lines);
  const uint32_t at = (i == 0 ? 1u : 0u) | (i == m - 1 ? 2u : 0u) | (j == 0 ? 4u : 0u) | (j == lines - 1 ? 8u : 0u);
  if (t >= (uint32_t)F.ntypes || (F.bits[t] & at) != 0) *bad = 1;
}
hipError_t launch_march_box_check(int64_t n, int m, int lines, const MarchForbid& F, const uint8_t* rtype,
                                  int32_t* bad, hipStream_t st) {
  if (m < 1 || lines < 1 || F.ntypes < 1 || F.ntypes > MARCH_TYPES || !rtype || !bad)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(march_box_check_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, m, lines,
                     F, rtype, bad);
  return hipGetLastError();
}

// ---- K-Strip: the multicolour smoother's whole leg of a NARROW level in one launch ----------
// Below the K-Patch levels (pitch < 128) the symmetric pass of a 4-colour level is 7 colour
// launches of ~5 us each with almost nothing to do, plus the residual + restriction or the
// prolongation: 16 launches per level and cycle.  Here a workgroup takes a strip of T consecutive
// rows plus a halo of (stages [+ 1]) x half-bandwidth rows on either side into LDS (u, f, row
// types, colours), runs the colour stages LDS -> LDS in place (rows of one colour do not read each
// other; a barrier between stages), and finishes with the residual + restriction (TAIL) or starts
// from u + P u_H (PROLONG): the 1-D counterpart of patch_rb_kernel, for any colouring (one colour
// byte per row).  The halo rows are recomputed by the neighbouring strips with the same
// expressions; row arithmetic = dict_rows<CSR_GS> / <CSR_RESID> on the level's own dictionary
// (ascending columns; the colour kernels walk the same entries of the symmetric matrix), transfers
// = patch_rb_kernel's: same bits as one launch per colour.
constexpr int STRIP_NT = 512;
constexpr int STRIP_WMAX = 4608;  // rows of a window (u and f: 2 x 36 KB of LDS)
typedef StripRef StripArgs;
int strip_window_max() { return STRIP_WMAX; }
template <int WORDS, int UN, bool PROLONG, bool TAIL>
__global__ __launch_bounds__(STRIP_NT) void mc_strip_kernel(StripArgs A) {
  __shared__ __attribute__((aligned(16))) double uw[STRIP_WMAX];
  __shared__ __attribute__((aligned(16))) double fw[STRIP_WMAX];
  __shared__ __attribute__((aligned(16))) uint8_t tyw[STRIP_WMAX];
  __shared__ __attribute__((aligned(16))) uint8_t cw8[STRIP_WMAX];
  __shared__ DictEntry tabG[256];
  __shared__ DictEntry tabR[TAIL ? 256 : 1];
  __shared__ uint64_t wtab[256 * WORDS];
  const int tid = (int)threadIdx.x;
  const int t0 = (int)blockIdx.x * A.T, w0 = t0 - A.H;
  const int W = A.T + 2 * A.H + 2;
  const int n = A.n;
  if (tid < 256) {
    dict_stage_table<CSR_GS>(tabG, A.doff, A.dval, A.ntab);
    if (TAIL) dict_stage_table<CSR_RESID>(tabR, A.doff, A.dval, A.ntab);
    dict_stage_words<WORDS>(wtab, A.rwords);
  }
  for (int lw = tid; lw < W; lw += STRIP_NT) {
    const int r = w0 + lw;
    const bool live = r >= 0 && r < n;
    const int row = live ? r : 0;
    double x0 = live ? A.x[row] : 0.0;
    if (PROLONG) {  // linear_prolong_add_kernel, same guards and order (patch_load)
      const int nH = A.nH;
      const int j = row >> 1;
      const bool odd = (row & 1) != 0;
      const bool a_ok = live && !odd && j >= 1 && j - 1 < nH;
      const bool b_ok = live && j < nH;
      const double a = A.uH[a_ok ? j - 1 : 0];
      const double b = A.uH[b_ok ? j : 0];
      double t = 0.0;
      t = a_ok ? t + 0.5 * a : t;
      t = b_ok ? t + (odd ? 1.0 : 0.5) * b : t;
      x0 = live ? x0 + t : x0;
    }
    uw[lw] = x0;
    fw[lw] = live ? A.f[row] : 0.0;
    tyw[lw] = live ? A.rtype[row] : (uint8_t)255;
    cw8[lw] = live ? A.color[row] : (uint8_t)255;
  }
  __syncthreads();
  constexpr int E = TAIL ? 1 : 0;
  for (int sg = 0; sg < A.nst; ++sg) {
    const uint32_t c = (uint32_t)(A.stages >> (4 * sg)) & 15u;
    const int ext = (A.nst - 1 - sg + E) * A.hbw;
    const int lo = A.H - ext, hi = A.H + A.T + 2 + ext;
    for (int lw = tid * 2; lw < W; lw += 2 * STRIP_NT) {
      DictStream<WORDS, 2> s;
      bool did[2];
      uint32_t ty = 0;
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int l = lw + r;
        did[r] = l >= lo && l < hi && (uint32_t)cw8[l] == c;
        s.live[r] = did[r];
        s.fi[r] = fw[l];
        s.xi[r] = uw[l];
        ty |= (did[r] ? (uint32_t)tyw[l] : 255u) << (8 * r);
      }
      s.ty = ty;
      dict_expand<WORDS, 2>(s, wtab);
      double res[2];
      dict_rows<CSR_GS, WORDS, UN, 2>(s, lw, tabG, uw, 1.0, 0, res);
      if (did[0]) uw[lw] = res[0];
      if (did[1]) uw[lw + 1] = res[1];
    }
    __syncthreads();
  }
  if (TAIL) {  // r = f - A u on the rows the restriction reads, left in the f window
    for (int lw = tid * 2; lw < W; lw += 2 * STRIP_NT) {
      DictStream<WORDS, 2> s;
      bool inr[2];
      uint32_t ty = 0;
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int l = lw + r;
        inr[r] = l >= A.H && l < A.H + A.T + 2 && tyw[l] != (uint8_t)255;
        s.live[r] = inr[r];
        s.fi[r] = fw[l];
        s.xi[r] = 0.0;
        ty |= (inr[r] ? (uint32_t)tyw[l] : 255u) << (8 * r);
      }
      s.ty = ty;
      dict_expand<WORDS, 2>(s, wtab);
      double res[2];
      dict_rows<CSR_RESID, WORDS, UN, 2>(s, lw, tabR, uw, 1.0, 0, res);
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int l = lw + r;
        if (l >= A.H && l < A.H + A.T + 2) fw[l] = inr[r] ? res[r] : 0.0;
      }
    }
    __syncthreads();
  }
  for (int q = tid; q < A.T; q += STRIP_NT) {
    const int r = t0 + q;
    if (r < n) {
      A.u_out[r] = uw[A.H + q];
      if (TAIL && A.r_out) A.r_out[r] = fw[A.H + q];
    }
  }
  if (TAIL) {
    for (int qj = tid; 2 * qj < A.T; qj += STRIP_NT) {
      const int64_t i = (int64_t)t0 + 2 * qj;  // fine row 2c
      const int64_t cj = i >> 1;
      if (i >= (int64_t)n || cj >= A.nH) continue;
      const double* rs = fw + A.H + 2 * qj;
      double sum = 0.0;  // dict_restrict_tail / linear_restrict_kernel, same guards and order
      if (i < n) sum += 0.5 * rs[0];
      if (i + 1 < n) sum += 1.0 * rs[1];
      if (i + 2 < n) sum += 0.5 * rs[2];
      A.fH[cj] = sum;
      if (A.uH_zero) A.uH_zero[cj] = 0.0;  // multigrid.hpp:278
    }
  }
}
bool strip_ok(const StripRef& A, const DictRef& D) {
  return D.rtype && D.rwords && D.doff && D.dval && dict_args_ok(A.n, D.words, D.wmax, D.ntab) && A.n >= 2 &&
         A.T >= 2 && (A.T & 1) == 0 && A.hbw >= D.hb && A.hbw >= 1 && A.nst >= 1 && A.nst <= 16 &&
         A.T + 2 * A.H + 2 <= STRIP_WMAX && A.color && A.x && A.f && A.u_out && A.u_out != A.x;
}
hipError_t launch_mc_strip(bool prolong, bool tail, StripRef A, const DictRef& D, hipStream_t st) {
  A.H = (A.nst + (tail ? 1 : 0)) * A.hbw;
  A.rtype = D.rtype; A.rwords = D.rwords; A.doff = D.doff; A.dval = D.dval; A.ntab = D.ntab;
  if (!strip_ok(A, D) || (prolong && (tail || !A.uH)) || (tail && !A.fH) || A.nH < 1) return hipErrorInvalidValue;
  const unsigned tiles = (unsigned)((A.n + A.T - 1) / A.T);
  return dict_dispatch_wu(D.words, D.wmax, [&](auto W, auto U) {
#define AMG_STRIP(PRO, TL) \
  hipLaunchKernelGGL((mc_strip_kernel<decltype(W)::value, decltype(U)::value, PRO, TL>), dim3(tiles), dim3(STRIP_NT), 0, st, A)
    if (tail) AMG_STRIP(false, true);
    else if (prolong) AMG_STRIP(true, false);
    else AMG_STRIP(false, false);
#undef AMG_STRIP
  });
}
void mc_strip_kernel_name(const DictRef& D, bool prolong, bool tail, char* buf, size_t cap) {
  dict_dispatch_class<0>(dict_wu_class(D.words, D.wmax), [&](auto W, auto U) {
    std::snprintf(buf, cap, "mc_strip_kernel<%d, %d, %s, %s>", (int)decltype(W)::value, (int)decltype(U)::value,
                  (prolong && !tail) ? "true" : "false", tail ? "true" : "false");
  });
}

void set_xcd_mapping(int on) {
  g_xcd_map = on ? 1 : 0;
  g_xcd_slab = on == 1 ? 1 : 0;  // 2: contiguous runs only (the round-2 order), an A/B switch
}
void set_dict_rows_per_lane(int r) { g_dict_rows_per_lane = r == 1 ? 1 : 2; }
void set_dict_stencil(int on) { g_dict_stencil = on ? 1 : 0; }
template <int MODE>
static hipError_t launch_dict_mode(int64_t n, const DictRef& D, const double* x, const double* f,
                                   double* out, double omega, int64_t dshift, hipStream_t st,
                                   double* dvec = nullptr, double alpha = 0.0) {
  const bool two = dict_two_rows(n, D, f, out);
  const unsigned tiles = (unsigned)((n + 256 * (two ? 2 : 1) - 1) / (256 * (two ? 2 : 1)));
  return dict_dispatch(D.words, D.wmax, D.nt != 0, two, [&](auto W, auto U, auto NTF, auto RR) {
    hipLaunchKernelGGL((dict_kernel<MODE, decltype(W)::value, decltype(U)::value,
                                    decltype(NTF)::value, decltype(RR)::value>),
                       dim3(tiles), dim3(256), 0, st, (int)n, D.codes, D.rtype, D.rwords, D.doff,
                       D.dval, D.ntab, x, f, out, omega, (int)dshift, dict_xcd_map(D, 256 * (two ? 2 : 1)),
                       dshift == 0 ? dict_stencil_tab(D, x) : nullptr, D.uti, dvec, alpha);
  });
}
hipError_t launch_dict_cheb(int64_t n, const DictRef& D, const double* x, const double* f, double* out,
                            const ChebStep& c, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  // d moves as 16-byte pairs when the rows do (dict_two_rows)
  if (!dict_args_ok(n, D.words, D.wmax, D.ntab) || !c.d || x == out ||
      (reinterpret_cast<uintptr_t>(c.d) & 15) != 0)
    return hipErrorInvalidValue;
#define AMG_DICT_CHEB(FI, LA) \
  return launch_dict_mode<cheb_kernel_mode(FI, LA)>(n, D, x, f, out, c.beta, 0, st, c.d, c.alpha)
  if (c.first && c.last) AMG_DICT_CHEB(true, true);
  if (c.first) AMG_DICT_CHEB(true, false);
  if (c.last) AMG_DICT_CHEB(false, true);
  AMG_DICT_CHEB(false, false);
#undef AMG_DICT_CHEB
}
// the name rocprofv3 prints for the launch launch_dict(mode, ...) makes
void dict_kernel_name(int mode, int64_t n, const DictRef& D, const void* f, const void* out,
                      char* buf, size_t cap) {
  const int u = D.words == 1 ? (D.wmax <= 3 ? 3 : D.wmax <= 5 ? 5 : D.wmax <= 7 ? 7 : 8)
                             : (D.wmax <= 9 ? 9 : D.wmax <= 12 ? 12 : 16);
  std::snprintf(buf, cap, "dict_kernel<%d, %d, %d, %s, %d>", mode, D.words, u,
                D.nt ? "true" : "false", dict_two_rows(n, D, f, out) ? 2 : 1);
}
hipError_t launch_dict(int mode, int64_t n, const DictRef& D, const double* x, const double* f,
                       double* out, double omega, int64_t diag_shift, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (!dict_args_ok(n, D.words, D.wmax, D.ntab) || diag_shift >= ((int64_t)1 << 28))
    return hipErrorInvalidValue;
  switch (mode) {
    case CSR_RESID: return launch_dict_mode<CSR_RESID>(n, D, x, f, out, omega, diag_shift, st);
    case CSR_JACOBI: return launch_dict_mode<CSR_JACOBI>(n, D, x, f, out, omega, diag_shift, st);
    case CSR_SPMV: return launch_dict_mode<CSR_SPMV>(n, D, x, f, out, omega, diag_shift, st);
    case CSR_RSSQ: return launch_dict_mode<CSR_RSSQ>(n, D, x, f, out, omega, diag_shift, st);
  }
  return hipErrorInvalidValue;
}

// ------------------------------------------------- K-Restrict / K-ProlongAdd ---
// f_H[j] = ((0 + 0.5 r[2j]) + 1.0 r[2j+1]) + 0.5 r[2j+2]   (Eigen column-major
// scatter order of R*v, interpolator.hpp:64-68 with R = P^T, :132-134).
// uH (optional) is zero-filled in the same pass (multigrid.hpp:278).
// T: double (the V-cycle) or float (K-F32, the single-precision preconditioner); the pair type of
// the 2-element lane accesses follows it.
template <class T> struct Pair;
template <> struct Pair<double> { using type = double2; };
template <> struct Pair<float> { using type = float2; };
template <class T>
static bool pair_aligned(const T* p) { return (reinterpret_cast<uintptr_t>(p) & (2 * sizeof(T) - 1)) == 0; }

template <class T>
__global__ __launch_bounds__(256) void linear_restrict_kernel(
    int64_t n_h, int64_t n_H, const T* __restrict__ r, T* __restrict__ fH,
    T* __restrict__ uH) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_H) return;
  if (uH) uH[j] = T(0.0);
  const int64_t i = 2 * j;
  T s = T(0.0);  // r is dead after this kernel: stream it
  if (i < n_h) s += T(0.5) * __builtin_nontemporal_load(r + i);
  if (i + 1 < n_h) s += T(1.0) * __builtin_nontemporal_load(r + i + 1);
  if (i + 2 < n_h) s += T(0.5) * r[i + 2];
  fH[j] = s;
}
// u_h[i] = u_h[i] + t[i], t = P u_H: t[2j+1] = 0 + 1.0 u_H[j];
// t[2j] = (0 + 0.5 u_H[j-1]) + 0.5 u_H[j]; rows past 2 n_H get t = 0
// (interpolator.hpp:52-56, multigrid.hpp:294-296).
template <class T>
__global__ __launch_bounds__(256) void linear_prolong_add_kernel(
    int64_t n_h, int64_t n_H, const T* __restrict__ uH, T* __restrict__ uh) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_h) return;
  T t = T(0.0);
  const int64_t j = i >> 1;
  if (i & 1) {
    if (j < n_H) t += T(1.0) * uH[j];
  } else {
    if (j >= 1 && j - 1 < n_H) t += T(0.5) * uH[j - 1];  // column j-1, row 2(j-1)+2
    if (j < n_H) t += T(0.5) * uH[j];                    // column j,   row 2j
  }
  uh[i] = uh[i] + t;
}
template <class T>
static hipError_t launch_linear_restrict_t(int64_t n_h, int64_t n_H, const T* r, T* fH, T* uH_zero,
                                           hipStream_t st) {
  if (n_H <= 0) return hipSuccess;
  hipLaunchKernelGGL(linear_restrict_kernel<T>, dim3((unsigned)((n_H + 255) / 256)),
                     dim3(256), 0, st, n_h, n_H, r, fH, uH_zero);
  return hipGetLastError();
}
hipError_t launch_linear_restrict(int64_t n_h, int64_t n_H, const double* r, double* fH,
                                  double* uH_zero, hipStream_t st) {
  return launch_linear_restrict_t<double>(n_h, n_H, r, fH, uH_zero, st);
}
// Two fine rows (2j, 2j+1) per lane: one pair load/store of u (16 bytes in double), same arithmetic.
template <class T>
__global__ __launch_bounds__(256) void linear_prolong_add2_kernel(
    int64_t n_h, int64_t n_H, const T* __restrict__ uH, const T* uh_in, T* uh) {
  using P2 = typename Pair<T>::type;
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t i = 2 * j;
  if (i >= n_h) return;
  T t0 = T(0.0), t1 = T(0.0);
  const T b = (j < n_H) ? uH[j] : T(0.0);
  if (j >= 1 && j - 1 < n_H) t0 += T(0.5) * uH[j - 1];
  if (j < n_H) {
    t0 += T(0.5) * b;
    t1 += T(1.0) * b;
  }
  if (i + 1 < n_h) {
    P2 u = *reinterpret_cast<const P2*>(uh_in + i);
    u.x = u.x + t0;
    u.y = u.y + t1;
    *reinterpret_cast<P2*>(uh + i) = u;
  } else {
    uh[i] = uh_in[i] + t0;
  }
}
// uh_out = uh_in + P uH (16-byte aligned vectors); uh_out == uh_in is the in-place form
hipError_t launch_linear_prolong_to(int64_t n_h, int64_t n_H, const double* uH,
                                    const double* uh_in, double* uh_out, hipStream_t st) {
  if (n_h <= 0) return hipSuccess;
  if (((reinterpret_cast<uintptr_t>(uh_in) | reinterpret_cast<uintptr_t>(uh_out)) & 15) != 0)
    return hipErrorInvalidValue;
  const int64_t nt = (n_h + 1) / 2;
  hipLaunchKernelGGL(linear_prolong_add2_kernel<double>, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0,
                     st, n_h, n_H, uH, uh_in, uh_out);
  return hipGetLastError();
}
template <class T>
static hipError_t launch_linear_prolong_add_t(int64_t n_h, int64_t n_H, const T* uH, T* uh, hipStream_t st) {
  if (n_h <= 0) return hipSuccess;
  if (pair_aligned(uh)) {
    const int64_t nt = (n_h + 1) / 2;
    hipLaunchKernelGGL(linear_prolong_add2_kernel<T>, dim3((unsigned)((nt + 255) / 256)), dim3(256),
                       0, st, n_h, n_H, uH, uh, uh);
  } else {
    hipLaunchKernelGGL(linear_prolong_add_kernel<T>, dim3((unsigned)((n_h + 255) / 256)),
                       dim3(256), 0, st, n_h, n_H, uH, uh);
  }
  return hipGetLastError();
}
hipError_t launch_linear_prolong_add(int64_t n_h, int64_t n_H, const double* uH,
                                     double* uh, hipStream_t st) {
  return launch_linear_prolong_add_t<double>(n_h, n_H, uH, uh, st);
}

// ------------------------------------- K-TensorRestrict / K-TensorProlong ---
// Full coarsening (host_setup.hpp: tensor_P): P = P1(nz) (x) P1(ny) (x) P1(nx), R = P^T, every axis
// m -> floor(m / 2), weights 0.5, 1.0, 0.5 on fine points 2J, 2J+1, 2J+2 (< m) of coarse point J.
// Semi-coarsening (the axis mask of tensor_P): an axis that is not coarsened keeps its length and
// contributes the identity -- one fine point J with weight 1.0 instead of three.
// All weights are products of powers of two, so every term w * v is exact and only the ORDER of
// the additions decides the bits: both kernels add in the order the CSR SpMV with R / P does.
// Natural boundary sides (amg_hip.h: opts->natural_sides; host_setup.hpp: tensor_P with sides): on a
// flagged side the boundary row of P1 carries 1.0 instead of 0.5 -- fine point 0 (low side), fine
// point n - 1 of an odd n (high side).  Still powers of two, the same terms in the same order.
// Periodic axes (amg_hip.h: amg_hip_create_tensor_periodic; host_setup.hpp: tensor_P with periodic):
// a coarsened periodic axis has an even length n >= 4 and P1per(n) = P1(n) plus the entry
// (0, n / 2 - 1) = 0.5.  Coarse point n / 2 - 1 then has the fine points 0, n - 2, n - 1 (ascending)
// with weights 0.5, 0.5, 1.0, and fine point 0 the coarse points 0 and n / 2 - 1, 0.5 each.  The
// kernels' PER instantiation knows the seam; PER = false is the code without it, unchanged.
struct TensorGrid {
  uint32_t nx, ny, nz;  // fine
  uint32_t mx, my, mz;  // coarse (m == n on an axis that is not coarsened)
  uint32_t cx, cy, cz;  // 1: the axis is coarsened
  uint32_t sides;       // bit 2a: low side of axis a is natural, bit 2a + 1: its high side
                        // bit 8 + a: axis a is periodic AND coarsened (its side bits are 0, n even, >= 4);
                        // kept in the same word so that the kernels' arguments lie where they lay
  __host__ __device__ uint32_t per() const { return sides >> 8; }
};
// P1N(2 J + t, J) on a coarsened axis of n fine points, t = 0, 1, 2; lo / hi: the axis' side bits
template <class T>
__device__ __forceinline__ T tn_weight(uint32_t J, uint32_t t, uint32_t n, uint32_t lo, uint32_t hi) {
  if (t == 1u) return T(1.0);
  if (t == 0u) return (lo && J == 0u) ? T(1.0) : T(0.5);
  return (hi && 2u * J + 3u == n) ? T(1.0) : T(0.5);
}

// One lane per coarse point (I, J, K): f_H = sum over k, j, i ascending (row order of R) of
// (wz wy wx) r[(k ny + j) nx + i], from +0.0.  The x-neighbours 2I, 2I+1 come as one aligned
// 16-byte load where the address allows (always, on rows of even length), 2I+2 as a scalar load of
// the line the next lane's pair sits in.  r is dead after this kernel.  VEC: r is 16-byte aligned
// (T = float, K-F32: the pair is 8 bytes and r 8-byte aligned; the weights are exact in float too).
// PER: the last coarse point of a periodic axis takes fine point 0 first (ascending fine index);
// on x that point is the first entry of the same line, a scalar load next to the pair (2I, 2I+1).
template <class T, bool VEC, bool PER>
__global__ __launch_bounds__(256) void tensor_restrict_kernel(
    TensorGrid g, const T* __restrict__ r, T* __restrict__ fH, T* __restrict__ uH) {
  using P2 = typename Pair<T>::type;
  const uint32_t nH = g.mx * g.my * g.mz;
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= nH) return;
  const uint32_t I = t % g.mx, q = t / g.mx, J = q % g.my, K = q / g.my;
  if (uH) uH[t] = T(0.0);
  const uint32_t i0 = g.cx ? 2u * I : I;  // cx: i0 + 1 < nx always (I < floor(nx / 2))
  const bool third = i0 + 2u < g.nx;
  const T wx0 = tn_weight<T>(I, 0u, g.nx, g.sides & 1u, g.sides & 2u);
  const T wx2 = tn_weight<T>(I, 2u, g.nx, g.sides & 1u, g.sides & 2u);
  // PER: this lane's coarse point is the last one of a periodic axis (2 m == n there, m >= 2)
  const bool seamx = PER && (g.per() & 1u) && i0 + 2u == g.nx;
  const bool seamy = PER && (g.per() & 2u) && 2u * J + 2u == g.ny;
  const bool seamz = PER && (g.per() & 4u) && 2u * K + 2u == g.nz;
  T s = T(0.0);
#pragma unroll
  for (uint32_t tz = 0; tz < 3; ++tz) {
    if (!g.cz && tz > 0) break;
    // seam: fine points 0, n - 2, n - 1 with weights 0.5, 0.5, 1.0
    const uint32_t k = seamz ? (tz == 0u ? 0u : 2u * K + tz - 1u) : (g.cz ? 2u * K + tz : K);
    if (k >= g.nz) break;
    const T wz = seamz ? (tz == 2u ? T(1.0) : T(0.5))
                       : (g.cz ? tn_weight<T>(K, tz, g.nz, g.sides & 16u, g.sides & 32u) : T(1.0));
#pragma unroll
    for (uint32_t ty = 0; ty < 3; ++ty) {
      if (!g.cy && ty > 0) break;
      const uint32_t j = seamy ? (ty == 0u ? 0u : 2u * J + ty - 1u) : (g.cy ? 2u * J + ty : J);
      if (j >= g.ny) break;
      const T w = wz * (seamy ? (ty == 2u ? T(1.0) : T(0.5))
                              : (g.cy ? tn_weight<T>(J, ty, g.ny, g.sides & 4u, g.sides & 8u) : T(1.0)));
      const int64_t a = ((int64_t)k * g.ny + j) * g.nx + i0;  // a + 1 (and a + 2 when third) < n_h
      if (!g.cx) {  // x is not coarsened: the one fine point I, neighbouring lanes read neighbours
        s += (w * T(1.0)) * r[a];
        continue;
      }
      T v0, v1, v2 = T(0.0);
      if (VEC && (a & 1) == 0) {
        const P2 p = *reinterpret_cast<const P2*>(r + a);
        v0 = p.x;
        v1 = p.y;
        if (third) v2 = r[a + 2];
      } else if (VEC && third) {
        v0 = r[a];
        const P2 p = *reinterpret_cast<const P2*>(r + a + 1);
        v1 = p.x;
        v2 = p.y;
      } else {
        v0 = r[a];
        v1 = r[a + 1];
        if (third) v2 = r[a + 2];
      }
      if (seamx) s += (w * T(0.5)) * r[a - i0];  // fine point 0 of this line (i0 = nx - 2, third is false)
      s += (w * wx0) * v0;
      s += (w * T(1.0)) * v1;
      if (third) s += (w * wx2) * v2;
    }
  }
  fH[t] = s;
}

// One lane per fine pair (2p, 2p+1) of a fine grid line: u_h += t, t = sum over K, J, I ascending
// (row order of P) of (wz wy wx) u_H[(K my + J) mx + I] from +0.0; 16-byte read-modify-write of
// u_h where the address allows.  An odd fine index has the one coarse neighbour (i - 1) / 2 with
// weight 1, an even one i / 2 - 1 and i / 2 with weight 0.5 (those that exist).  On an axis that is
// not coarsened a fine point has the one coarse neighbour of its own index with weight 1; along x
// the lane's fine pair then reads the coarse pair (2p, 2p+1), 16 bytes where that address allows.
// PER: fine point 0 of a periodic axis has the coarse neighbours 0 and m - 1, in that order, 0.5
// each; on x that is lane p = 0 of every line, whose wrapped term comes after the `mid` term.
template <class T, bool VEC, bool PER>
__global__ __launch_bounds__(256) void tensor_prolong_add_kernel(
    TensorGrid g, const T* __restrict__ uH, T* uh) {
  using P2 = typename Pair<T>::type;
  const uint32_t px = (g.nx + 1u) / 2u;  // pairs per fine line
  const uint32_t total = px * g.ny * g.nz;
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= total) return;
  const uint32_t p = t % px, row = t / px, j = row % g.ny, k = row / g.ny;
  // coarse neighbours along y and z: (index, weight, exists), ascending
  uint32_t Jc[2], Kc[2];
  T wy[2], wz[2];
  bool oky[2], okz[2];
  if (!g.cy) {
    Jc[0] = j; wy[0] = 1.0; oky[0] = true;
    Jc[1] = 0; wy[1] = 0.0; oky[1] = false;
  } else if (PER && (g.per() & 2u) && j == 0u) {
    Jc[0] = 0; wy[0] = 0.5; oky[0] = true;
    Jc[1] = g.my - 1u; wy[1] = 0.5; oky[1] = true;  // my >= 2
  } else if (j & 1u) {
    Jc[0] = (j - 1u) / 2u; wy[0] = 1.0; oky[0] = Jc[0] < g.my;
    Jc[1] = 0; wy[1] = 0.0; oky[1] = false;
  } else {
    Jc[0] = j / 2u - 1u; wy[0] = ((g.sides & 8u) && j + 1u == g.ny) ? 1.0 : 0.5; oky[0] = j >= 2u && Jc[0] < g.my;
    Jc[1] = j / 2u; wy[1] = ((g.sides & 4u) && j == 0u) ? 1.0 : 0.5; oky[1] = Jc[1] < g.my;
  }
  if (!g.cz) {
    Kc[0] = k; wz[0] = 1.0; okz[0] = true;
    Kc[1] = 0; wz[1] = 0.0; okz[1] = false;
  } else if (PER && (g.per() & 4u) && k == 0u) {
    Kc[0] = 0; wz[0] = 0.5; okz[0] = true;
    Kc[1] = g.mz - 1u; wz[1] = 0.5; okz[1] = true;  // mz >= 2
  } else if (k & 1u) {
    Kc[0] = (k - 1u) / 2u; wz[0] = 1.0; okz[0] = Kc[0] < g.mz;
    Kc[1] = 0; wz[1] = 0.0; okz[1] = false;
  } else {
    Kc[0] = k / 2u - 1u; wz[0] = ((g.sides & 32u) && k + 1u == g.nz) ? 1.0 : 0.5; okz[0] = k >= 2u && Kc[0] < g.mz;
    Kc[1] = k / 2u; wz[1] = ((g.sides & 16u) && k == 0u) ? 1.0 : 0.5; okz[1] = Kc[1] < g.mz;
  }
  const bool left = g.cx && p >= 1u && p - 1u < g.mx;  // coarse I = p - 1 feeds fine 2p
  const bool mid = g.cx && p < g.mx;                   // coarse I = p feeds fine 2p and 2p + 1
  const bool two = 2u * p + 1u < g.nx;                 // the lane's pair is whole
  const bool wrap = PER && (g.per() & 1u) && p == 0u;    // coarse I = mx - 1 feeds fine 0 (mx >= 2: mid holds)
  // fine 2p is the last point of an odd line / the first point: the natural sides' weight 1
  const T wl = ((g.sides & 2u) && 2u * p + 1u == g.nx) ? T(1.0) : T(0.5);
  const T wm = ((g.sides & 1u) && p == 0u) ? T(1.0) : T(0.5);
  T t0 = T(0.0), t1 = T(0.0);
#pragma unroll
  for (int a = 0; a < 2; ++a) {
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      if (okz[a] && oky[b]) {
        const T w = wz[a] * wy[b];
        const T* c = uH + ((int64_t)Kc[a] * g.my + Jc[b]) * g.mx;
        if (!g.cx) {  // mx == nx: coarse 2p feeds fine 2p, coarse 2p + 1 fine 2p + 1
          const T* c2 = c + 2u * p;
          if (VEC && two && (reinterpret_cast<uintptr_t>(c2) & (sizeof(P2) - 1u)) == 0) {
            const P2 m = *reinterpret_cast<const P2*>(c2);
            t0 += (w * T(1.0)) * m.x;
            t1 += (w * T(1.0)) * m.y;
          } else {
            t0 += (w * T(1.0)) * c2[0];
            if (two) t1 += (w * T(1.0)) * c2[1];
          }
        }
        if (left) t0 += (w * wl) * c[p - 1u];
        if (mid) {
          const T m = c[p];
          t0 += (w * wm) * m;
          t1 += (w * T(1.0)) * m;
        }
        if (wrap) t0 += (w * T(0.5)) * c[g.mx - 1u];
      }
    }
  }
  const int64_t i = (int64_t)row * g.nx + 2u * p;
  if (two) {
    if (VEC && (i & 1) == 0) {
      P2 u = *reinterpret_cast<const P2*>(uh + i);
      u.x = u.x + t0;
      u.y = u.y + t1;
      *reinterpret_cast<P2*>(uh + i) = u;
    } else {
      uh[i] = uh[i] + t0;
      uh[i + 1] = uh[i + 1] + t1;
    }
  } else {
    uh[i] = uh[i] + t0;
  }
}

static bool tensor_grid(int dim, const int64_t dims[3], uint32_t mask, uint32_t sides, uint32_t periodic,
                        TensorGrid* g) {
  if ((dim != 2 && dim != 3) || !dims) return false;
  if (sides >= (1u << (2 * dim))) return false;
  if (periodic >= (1u << dim)) return false;
  for (int a = 0; a < dim; ++a)  // a periodic axis has no sides; coarsened, it is even and >= 4
    if ((periodic >> a) & 1u) {
      if ((sides >> (2 * a)) & 3u) return false;
      if (((mask >> a) & 1u) && (dims[a] < 4 || (dims[a] & 1))) return false;
    }
  g->sides = sides | ((periodic & mask) << 8);
  if (mask == 0u || mask > (dim == 3 ? 7u : 3u)) return false;
  const int64_t nx = dims[0], ny = dims[1], nz = dim == 3 ? dims[2] : 1;
  if (nx < 1 || ny < 1 || nz < 1 || (dim == 2 && dims[2] != 1)) return false;
  g->cx = mask & 1u;
  g->cy = (mask >> 1) & 1u;
  g->cz = (mask >> 2) & 1u;
  if ((g->cx && nx < 2) || (g->cy && ny < 2) || (g->cz && nz < 2)) return false;
  if (nx >= ((int64_t)1 << 31) / ny / nz - 2) return false;  // 32-bit lane indices
  g->nx = (uint32_t)nx;
  g->ny = (uint32_t)ny;
  g->nz = (uint32_t)nz;
  g->mx = (uint32_t)(g->cx ? nx / 2 : nx);
  g->my = (uint32_t)(g->cy ? ny / 2 : ny);
  g->mz = (uint32_t)(g->cz ? nz / 2 : nz);
  return true;
}
template <class T>
static hipError_t launch_tensor_restrict_t(int dim, const int64_t dims[3], uint32_t mask, uint32_t sides, uint32_t periodic,
                                           const T* r, T* fH, T* uH_zero, hipStream_t st) {
  TensorGrid g;
  if (!tensor_grid(dim, dims, mask, sides, periodic, &g)) return hipErrorInvalidValue;
  const uint32_t nH = g.mx * g.my * g.mz;
  const dim3 grid((nH + 255u) / 256u), block(256);
  if (g.per()) {  // a seam on a coarsened axis
    if (pair_aligned(r))
      hipLaunchKernelGGL((tensor_restrict_kernel<T, true, true>), grid, block, 0, st, g, r, fH, uH_zero);
    else
      hipLaunchKernelGGL((tensor_restrict_kernel<T, false, true>), grid, block, 0, st, g, r, fH, uH_zero);
  } else if (pair_aligned(r))
    hipLaunchKernelGGL((tensor_restrict_kernel<T, true, false>), grid, block, 0, st, g, r, fH, uH_zero);
  else
    hipLaunchKernelGGL((tensor_restrict_kernel<T, false, false>), grid, block, 0, st, g, r, fH, uH_zero);
  return hipGetLastError();
}
hipError_t launch_tensor_restrict(int dim, const int64_t dims[3], uint32_t mask, uint32_t sides, uint32_t periodic,
                                  const double* r, double* fH, double* uH_zero, hipStream_t st) {
  return launch_tensor_restrict_t<double>(dim, dims, mask, sides, periodic, r, fH, uH_zero, st);
}
template <class T>
static hipError_t launch_tensor_prolong_add_t(int dim, const int64_t dims[3], uint32_t mask, uint32_t sides, uint32_t periodic,
                                              const T* uH, T* uh, hipStream_t st) {
  TensorGrid g;
  if (!tensor_grid(dim, dims, mask, sides, periodic, &g)) return hipErrorInvalidValue;
  const uint32_t total = ((g.nx + 1u) / 2u) * g.ny * g.nz;
  const dim3 grid((total + 255u) / 256u), block(256);
  if (g.per()) {
    if (pair_aligned(uh))
      hipLaunchKernelGGL((tensor_prolong_add_kernel<T, true, true>), grid, block, 0, st, g, uH, uh);
    else
      hipLaunchKernelGGL((tensor_prolong_add_kernel<T, false, true>), grid, block, 0, st, g, uH, uh);
  } else if (pair_aligned(uh))
    hipLaunchKernelGGL((tensor_prolong_add_kernel<T, true, false>), grid, block, 0, st, g, uH, uh);
  else
    hipLaunchKernelGGL((tensor_prolong_add_kernel<T, false, false>), grid, block, 0, st, g, uH, uh);
  return hipGetLastError();
}
hipError_t launch_tensor_prolong_add(int dim, const int64_t dims[3], uint32_t mask, uint32_t sides, uint32_t periodic,
                                     const double* uH, double* uh, hipStream_t st) {
  return launch_tensor_prolong_add_t<double>(dim, dims, mask, sides, periodic, uH, uh, st);
}

// ----------------------------------------- K-AxisRestrict / K-AxisProlong ---
// One coarsened axis per level, weights from the level's matrix (kernels.hpp: launch_axis_restrict;
// host_setup.hpp: axis_opdep_P).  Coarse point H of the axis sits at fine coordinate 2 H + 1; column
// H of P holds w_hi(2 H), 1.0, w_lo(2 H + 2) on the fine coordinates 2 H, 2 H + 1, 2 H + 2 (< m).
// The weights are arbitrary doubles, so each product rounds (-ffp-contract=off keeps it apart from
// the addition) and the sums run in the order of csr_stage_kernel on R / P: from +0.0, ascending column.
struct AxisGrid {
  uint32_t nx, ny, nz;  // fine
  uint32_t m, mH, mE;   // the axis: fine length, coarse length floor(m / 2), even points m - mH
};
// the 16-byte pair (c[0], c[1]) where the address allows, c[1] only when `two`
template <bool VEC>
__device__ __forceinline__ void axis_load2(const double* c, bool two, double& v0, double& v1) {
  if (VEC && two && (reinterpret_cast<uintptr_t>(c) & 15u) == 0) {
    const double2 p = *reinterpret_cast<const double2*>(c);
    v0 = p.x;
    v1 = p.y;
  } else {
    v0 = c[0];
    v1 = two ? c[1] : 0.0;
  }
}

// One lane per coarse point: f_H = ((+0.0 + w_hi(2H) r(2H)) + 1.0 r(2H+1)) + w_lo(2H+2) r(2H+2), the
// last term when 2H + 2 < m.  Along x the fine points 2I, 2I+1 come as one aligned 16-byte load
// where the address allows (VEC: r is 16-byte aligned), as in tensor_restrict_kernel; along y / z
// the three loads of a wave are contiguous lines.  The two weights are the second half of W's pair
// e and the first half of pair e + stride.  uH (may be null) is zeroed in the same pass.
// PER: the axis wraps (m even, >= 4; mE = mH = m / 2).  The third point of the last coarse point
// H = mH - 1 is fine 0, the lowest row of its column of P, so there the sum runs
// ((+0.0 + w_lo(0) r(0)) + w_hi(m-2) r(m-2)) + 1.0 r(m-1); its weight is the first half of the line's
// pair 0 and its value a scalar load from the other end of the line (along y / z: of the axis, a
// contiguous line).  Every other H keeps the order above, and the third term always exists.
template <int AXIS, bool VEC, bool PER = false>
__global__ __launch_bounds__(256) void axis_restrict_kernel(
    AxisGrid g, const double* __restrict__ W, const double* __restrict__ r, double* __restrict__ fH,
    double* __restrict__ uH) {
  const uint32_t cx = AXIS == 0 ? g.mH : g.nx, cy = AXIS == 1 ? g.mH : g.ny, cz = AXIS == 2 ? g.mH : g.nz;
  const uint32_t nH = cx * cy * cz;
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= nH) return;
  const uint32_t I = t % cx, q = t / cx, J = q % cy, K = q / cy;
  if (uH) uH[t] = 0.0;
  const uint32_t H = AXIS == 0 ? I : (AXIS == 1 ? J : K);
  const bool third = PER || 2u * H + 2u < g.m;
  const bool seam = PER && 2u * H + 2u == g.m;
  int64_t a, e, sd;  // fine index of coordinate 2 H, index of that even point, stride of the axis in both
  if (AXIS == 0) {
    a = ((int64_t)K * g.ny + J) * g.nx + 2u * I;
    e = ((int64_t)K * g.ny + J) * g.mE + I;
    sd = 1;
  } else if (AXIS == 1) {
    a = ((int64_t)K * g.ny + 2u * J) * g.nx + I;
    e = ((int64_t)K * g.mE + J) * g.nx + I;
    sd = g.nx;
  } else {
    a = ((int64_t)2u * K * g.ny + J) * g.nx + I;
    e = ((int64_t)K * g.ny + J) * g.nx + I;
    sd = (int64_t)g.nx * g.ny;
  }
  // the third point and its even point: two steps up the axis, or H (2 H) steps down to fine 0
  const int64_t a2 = seam ? a - (int64_t)(2u * H) * sd : a + 2 * sd;
  const int64_t e2 = seam ? e - (int64_t)H * sd : e + sd;
  const double whi = W[2 * e + 1];
  const double wlo = third ? W[2 * e2] : 0.0;
  double v0, v1, v2 = 0.0;
  if (AXIS == 0 && VEC && (a & 1) == 0) {
    const double2 p = *reinterpret_cast<const double2*>(r + a);
    v0 = p.x;
    v1 = p.y;
    if (third) v2 = r[a2];
  } else if (AXIS == 0 && VEC && third && !seam) {
    v0 = r[a];
    const double2 p = *reinterpret_cast<const double2*>(r + a + 1);
    v1 = p.x;
    v2 = p.y;
  } else {
    v0 = r[a];
    v1 = r[a + sd];
    if (third) v2 = r[a2];
  }
  double s = 0.0;
  if (seam) {
    s += wlo * v2;
    s += whi * v0;
    s += 1.0 * v1;
  } else {
    s += whi * v0;
    s += 1.0 * v1;
    if (third) s += wlo * v2;
  }
  fH[t] = s;
}

// One lane per fine pair (2p, 2p+1) of a fine grid line: u_h += t with t summed from +0.0 over the
// coarse neighbours in ascending order; 16-byte read-modify-write of u_h where the address allows
// (VEC: u_h, u_H and W are 16-byte aligned).  An odd axis coordinate c has the one coarse neighbour
// (c - 1) / 2 with weight 1.0; an even one c / 2 - 1 with w_lo (c >= 2) and c / 2 with w_hi
// (c + 1 < m), one 16-byte load of W per fine point.  Along x the lane's even point is 2p and its
// odd one 2p + 1; along y / z both points of the pair have the lane's c and read coarse pairs.
// PER: the axis wraps (m even, >= 4; mE = mH = m / 2), so every even c has both neighbours, the low
// one (c / 2 - 1) mod mH.  At c = 0 that is the LAST coarse point, and the ascending order puts the
// high term first: t = (+0.0 + w_hi(0) u_H(0)) + w_lo(0) u_H(mH - 1) -- along x a scalar load from
// the other end of the coarse line in lane p = 0, along y / z a contiguous coarse line.
template <int AXIS, bool VEC, bool PER = false>
__global__ __launch_bounds__(256) void axis_prolong_add_kernel(
    AxisGrid g, const double2* __restrict__ W, const double* __restrict__ uH, double* uh) {
  const uint32_t px = (g.nx + 1u) / 2u;  // pairs per fine line
  const uint32_t total = px * g.ny * g.nz;
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= total) return;
  const uint32_t p = t % px, row = t / px, j = row % g.ny, k = row / g.ny;
  const bool two = 2u * p + 1u < g.nx;  // the lane's pair is whole
  double t0 = 0.0, t1 = 0.0;
  if (AXIS == 0) {  // mE == px: the even point of the pair is point p of the line's even points
    const double2 w = W[(int64_t)row * g.mE + p];
    const double* c = uH + (int64_t)row * g.mH;
    if (PER) {  // nx = m is even: the pair is whole and coarse p exists
      const double mid = c[p];
      if (p == 0u) {
        t0 += w.y * mid;
        t0 += w.x * c[g.mH - 1u];
      } else {
        t0 += w.x * c[p - 1u];
        t0 += w.y * mid;
      }
      t1 += 1.0 * mid;
    } else {
      if (p >= 1u) t0 += w.x * c[p - 1u];
      if (two) {  // coarse p exists iff fine 2p + 1 does
        const double mid = c[p];
        t0 += w.y * mid;
        t1 += 1.0 * mid;
      }
    }
  } else {
    const uint32_t cc = AXIS == 1 ? j : k;
    // coarse / even-grid index of the lane's x = 2p on the line with axis coordinate h
    auto base = [&](uint32_t len, uint32_t h) -> int64_t {
      return (AXIS == 1 ? ((int64_t)k * len + h) : ((int64_t)h * g.ny + j)) * g.nx + 2u * p;
    };
    double m0, m1;
    if (cc & 1u) {
      axis_load2<VEC>(uH + base(g.mH, (cc - 1u) / 2u), two, m0, m1);
      t0 += 1.0 * m0;
      if (two) t1 += 1.0 * m1;
    } else {
      const uint32_t h = cc / 2u;
      const int64_t e = base(g.mE, h);
      const double2 w0 = W[e];
      const double2 w1 = two ? W[e + 1] : make_double2(0.0, 0.0);
      if (PER && cc == 0u) {  // the seam line: high first, then the low neighbour on the last coarse line
        axis_load2<VEC>(uH + base(g.mH, 0u), two, m0, m1);
        t0 += w0.y * m0;
        if (two) t1 += w1.y * m1;
        axis_load2<VEC>(uH + base(g.mH, g.mH - 1u), two, m0, m1);
        t0 += w0.x * m0;
        if (two) t1 += w1.x * m1;
      } else {
        if (cc >= 2u) {
          axis_load2<VEC>(uH + base(g.mH, h - 1u), two, m0, m1);
          t0 += w0.x * m0;
          if (two) t1 += w1.x * m1;
        }
        if (cc + 1u < g.m) {
          axis_load2<VEC>(uH + base(g.mH, h), two, m0, m1);
          t0 += w0.y * m0;
          if (two) t1 += w1.y * m1;
        }
      }
    }
  }
  const int64_t i = (int64_t)row * g.nx + 2u * p;
  if (two) {
    if (VEC && (i & 1) == 0) {
      double2 u = *reinterpret_cast<const double2*>(uh + i);
      u.x = u.x + t0;
      u.y = u.y + t1;
      *reinterpret_cast<double2*>(uh + i) = u;
    } else {
      uh[i] = uh[i] + t0;
      uh[i + 1] = uh[i + 1] + t1;
    }
  } else {
    uh[i] = uh[i] + t0;
  }
}

static bool axis_grid(int dim, const int64_t dims[3], int axis, AxisGrid* g) {
  if ((dim != 2 && dim != 3) || !dims || axis < 0 || axis >= dim) return false;
  const int64_t nx = dims[0], ny = dims[1], nz = dim == 3 ? dims[2] : 1;
  if (nx < 1 || ny < 1 || nz < 1 || (dim == 2 && dims[2] != 1) || dims[axis] < 2) return false;
  if (nx >= ((int64_t)1 << 31) / ny / nz - 2) return false;  // 32-bit lane indices
  g->nx = (uint32_t)nx;
  g->ny = (uint32_t)ny;
  g->nz = (uint32_t)nz;
  g->m = (uint32_t)dims[axis];
  g->mH = g->m / 2u;
  g->mE = g->m - g->mH;
  return true;
}
hipError_t launch_axis_restrict(int dim, const int64_t dims[3], int axis, bool periodic, const double* W,
                                const double* r, double* fH, double* uH_zero, hipStream_t st) {
  AxisGrid g;
  if (!axis_grid(dim, dims, axis, &g) || !pair_aligned(W)) return hipErrorInvalidValue;
  if (periodic && (g.m < 4u || (g.m & 1u))) return hipErrorInvalidValue;
  const uint32_t nH = g.nx * g.ny * g.nz / g.m * g.mH;
  const dim3 grid((nH + 255u) / 256u), block(256);
  if (periodic) {  // the seam forms, beside the open ones below
    if (axis == 0) {
      if (pair_aligned(r))
        hipLaunchKernelGGL((axis_restrict_kernel<0, true, true>), grid, block, 0, st, g, W, r, fH, uH_zero);
      else
        hipLaunchKernelGGL((axis_restrict_kernel<0, false, true>), grid, block, 0, st, g, W, r, fH, uH_zero);
    } else if (axis == 1) {
      hipLaunchKernelGGL((axis_restrict_kernel<1, false, true>), grid, block, 0, st, g, W, r, fH, uH_zero);
    } else {
      hipLaunchKernelGGL((axis_restrict_kernel<2, false, true>), grid, block, 0, st, g, W, r, fH, uH_zero);
    }
    return hipGetLastError();
  }
  if (axis == 0) {
    if (pair_aligned(r))
      hipLaunchKernelGGL((axis_restrict_kernel<0, true>), grid, block, 0, st, g, W, r, fH, uH_zero);
    else
      hipLaunchKernelGGL((axis_restrict_kernel<0, false>), grid, block, 0, st, g, W, r, fH, uH_zero);
  } else if (axis == 1) {
    hipLaunchKernelGGL((axis_restrict_kernel<1, false>), grid, block, 0, st, g, W, r, fH, uH_zero);
  } else {
    hipLaunchKernelGGL((axis_restrict_kernel<2, false>), grid, block, 0, st, g, W, r, fH, uH_zero);
  }
  return hipGetLastError();
}
hipError_t launch_axis_prolong_add(int dim, const int64_t dims[3], int axis, bool periodic, const double* W,
                                   const double* uH, double* uh, hipStream_t st) {
  AxisGrid g;
  if (!axis_grid(dim, dims, axis, &g) || !pair_aligned(W)) return hipErrorInvalidValue;
  if (periodic && (g.m < 4u || (g.m & 1u))) return hipErrorInvalidValue;
  const uint32_t total = ((g.nx + 1u) / 2u) * g.ny * g.nz;
  const dim3 grid((total + 255u) / 256u), block(256);
  const double2* W2 = reinterpret_cast<const double2*>(W);
  const bool vec = pair_aligned(uh) && pair_aligned(uH);
#define AMG_AXIS_PROLONG(AX, PER)                                                                              \
  if (vec) hipLaunchKernelGGL((axis_prolong_add_kernel<AX, true, PER>), grid, block, 0, st, g, W2, uH, uh);   \
  else hipLaunchKernelGGL((axis_prolong_add_kernel<AX, false, PER>), grid, block, 0, st, g, W2, uH, uh)
  if (periodic) {
    if (axis == 0) { AMG_AXIS_PROLONG(0, true); }
    else if (axis == 1) { AMG_AXIS_PROLONG(1, true); }
    else { AMG_AXIS_PROLONG(2, true); }
  } else if (axis == 0) { AMG_AXIS_PROLONG(0, false); }
  else if (axis == 1) { AMG_AXIS_PROLONG(1, false); }
  else { AMG_AXIS_PROLONG(2, false); }
#undef AMG_AXIS_PROLONG
  return hipGetLastError();
}

// First Jacobi sweep from a zero guess (coarse levels on the way down,
// multigrid.hpp:278 then :268): with u == 0 every a_ij*u_j is +-0 and the row sum
// is +0.0, so the sweep needs only f and the diagonal -- same operations, same
// bits as the full kernel on a zero vector, without streaming the matrix.
__global__ __launch_bounds__(256) void jacobi_from_zero_kernel(
    int64_t n, const double* __restrict__ diag, const double* __restrict__ f,
    double* __restrict__ out, double omega) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double xi = 0.0, acc = 0.0;
  const double d = diag[i], fi = f[i];
  out[i] = (d == 0.0) ? xi : xi + omega * ((fi - acc) / d - xi);
}
hipError_t launch_jacobi_from_zero(int64_t n, const double* diag, const double* f, double* out,
                                   double omega, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(jacobi_from_zero_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     st, n, diag, f, out, omega);
  return hipGetLastError();
}

// x[j * stride] = +0.0, j < count (count <= 64): the pinned entry of the coarsest right-hand side of a
// singular solver (solver.cpp: launch_coarse), one per column in the block cycle: all columns of a
// panel in one launch.
__global__ __launch_bounds__(64) void zero_strided_kernel(double* __restrict__ x, int64_t stride, int count) {
  if ((int)threadIdx.x < count) x[(int64_t)threadIdx.x * stride] = 0.0;
}
hipError_t launch_zero_strided(double* x, int64_t stride, int count, hipStream_t st) {
  if (count <= 0) return hipSuccess;
  if (count > 64 || !x) return hipErrorInvalidValue;
  hipLaunchKernelGGL(zero_strided_kernel, dim3(1), dim3(64), 0, st, x, stride, count);
  return hipGetLastError();
}

__global__ __launch_bounds__(256) void add_inplace_kernel(int64_t n,
                                                          const double* __restrict__ x,
                                                          double* __restrict__ y) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = y[i] + x[i];
}
hipError_t launch_add_inplace(int64_t n, const double* x, double* y, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(add_inplace_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     st, n, x, y);
  return hipGetLastError();
}

// ---------------------------------------------------------------- K-SumSq ----
// Deterministic two-stage reduction: grid-stride per-thread sums, wave shuffle
// tree, LDS across the 4 waves, one partial per block; the last stage is one
// block over <= 1024 partials.  square=1: sum of x^2, square=0: plain sum.
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}
__global__ __launch_bounds__(256) void sum_kernel(int64_t n, const double* __restrict__ x,
                                                  double* __restrict__ out, int square) {
  __shared__ double part[4];
  double s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const double v = x[i];
    s += square ? v * v : v;
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[blockIdx.x] = ((part[0] + part[1]) + part[2]) + part[3];
}
hipError_t launch_sum(int64_t n, const double* x, double* out, double* scratch, int square,
                      hipStream_t st) {
  int64_t g = (n + 255) / 256;
  if (g > 1024) g = 1024;
  if (g < 1) g = 1;
  hipLaunchKernelGGL(sum_kernel, dim3((unsigned)g), dim3(256), 0, st, n, x, scratch, square);
  hipLaunchKernelGGL(sum_kernel, dim3(1), dim3(256), 0, st, g, scratch, out, 0);
  return hipGetLastError();
}

// ------------------------------------------------------------------ K-PCG -----
// Vector kernels of the preconditioned conjugate-gradient driver (the V-cycle as M^-1,
// README.md:127 of the reference): deterministic two-stage dot product and the two
// updates; the scalars alpha / beta are formed on the device from the dot products in
// sc[], so an iteration needs no host round trip.
__global__ __launch_bounds__(256) void dot_kernel(int64_t n, const double* __restrict__ x,
                                                  const double* __restrict__ y,
                                                  double* __restrict__ out) {
  __shared__ double part[4];
  double s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    s += x[i] * y[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[blockIdx.x] = ((part[0] + part[1]) + part[2]) + part[3];
}
hipError_t launch_dot(int64_t n, const double* x, const double* y, double* out, double* scratch,
                      hipStream_t st) {
  int64_t g = (n + 255) / 256;
  if (g > 1024) g = 1024;
  if (g < 1) g = 1;
  hipLaunchKernelGGL(dot_kernel, dim3((unsigned)g), dim3(256), 0, st, n, x, y, scratch);
  hipLaunchKernelGGL(sum_kernel, dim3(1), dim3(256), 0, st, g, scratch, out, 0);
  return hipGetLastError();
}
// alpha = num / den;  x = x + alpha p;  r = r - alpha q
__global__ __launch_bounds__(256) void pcg_update_xr_kernel(int64_t n, const double* __restrict__ num,
                                                            const double* __restrict__ den, double* x,
                                                            double* r, const double* __restrict__ p,
                                                            const double* __restrict__ q) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double alpha = *num / *den;
  x[i] = x[i] + alpha * p[i];
  r[i] = r[i] - alpha * q[i];
}
// beta = num / den;  p = z + beta p
__global__ __launch_bounds__(256) void pcg_update_p_kernel(int64_t n, const double* __restrict__ num,
                                                           const double* __restrict__ den, double* p,
                                                           const double* __restrict__ z) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double beta = *num / *den;
  p[i] = z[i] + beta * p[i];
}
hipError_t launch_pcg_update_xr(int64_t n, const double* num, const double* den, double* x, double* r,
                                const double* p, const double* q, hipStream_t st) {
  hipLaunchKernelGGL(pcg_update_xr_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, num,
                     den, x, r, p, q);
  return hipGetLastError();
}
hipError_t launch_pcg_update_p(int64_t n, const double* num, const double* den, double* p,
                               const double* z, hipStream_t st) {
  hipLaunchKernelGGL(pcg_update_p_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, num,
                     den, p, z);
  return hipGetLastError();
}

// --------------------------------------------------------------- K-Center ----
// Mean projection of the PCG drivers on singular solvers (amg_hip_set_mean_projection):
// centre(v)_i = v_i - m with m = *sum / (double)n, one IEEE divide of launch_sum's device scalar
// and one subtract per entry.
// center_kernel: dst = centre(src), dst may be src.  Element-wise, so a lane takes two neighbours
// in one 16-byte access (PAIRS; both pointers 16-byte aligned) and the odd last entry goes to the
// thread after the last pair.
template <bool PAIRS>
__global__ __launch_bounds__(256) void center_kernel(int64_t n, const double* __restrict__ sum, const double* src,
                                                     double* dst) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const double m = *sum / (double)n;
  if (PAIRS) {
    const int64_t np = n >> 1;
    if (e < np) {
      double2 v = reinterpret_cast<const double2*>(src)[e];
      v.x = v.x - m;
      v.y = v.y - m;
      reinterpret_cast<double2*>(dst)[e] = v;
    } else if (e == np && (n & 1)) {
      dst[n - 1] = src[n - 1] - m;
    }
  } else {
    if (e < n) dst[e] = src[e] - m;
  }
}
hipError_t launch_center(int64_t n, const double* sum, const double* src, double* dst, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if ((((uintptr_t)src | (uintptr_t)dst) & 15) == 0) {
    const int64_t threads = (n >> 1) + (n & 1);
    hipLaunchKernelGGL(center_kernel<true>, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, n, sum, src,
                       dst);
  } else {
    hipLaunchKernelGGL(center_kernel<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, sum, src, dst);
  }
  return hipGetLastError();
}
// center_dot_kernel: z = centre(z) and the first stage of r . z in one pass: dot_kernel's grid,
// grid-stride order and tree with the term r[i] * (z[i] - m), so the partials -- and after
// sum_kernel the result -- have the bits of launch_dot(r, centre(z)).  The tree hands entry i to
// thread i mod G, which leaves one entry per lane and access.
__global__ __launch_bounds__(256) void center_dot_kernel(int64_t n, const double* __restrict__ sum,
                                                         double* __restrict__ z, const double* __restrict__ r,
                                                         double* __restrict__ out) {
  __shared__ double part[4];
  const double m = *sum / (double)n;
  double s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const double zc = z[i] - m;
    z[i] = zc;
    s += r[i] * zc;
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[blockIdx.x] = ((part[0] + part[1]) + part[2]) + part[3];
}
hipError_t launch_center_dot(int64_t n, const double* sum, double* z, const double* r, double* out,
                             double* scratch, hipStream_t st) {
  int64_t g = (n + 255) / 256;
  if (g > 1024) g = 1024;
  if (g < 1) g = 1;
  hipLaunchKernelGGL(center_dot_kernel, dim3((unsigned)g), dim3(256), 0, st, n, sum, z, r, scratch);
  hipLaunchKernelGGL(sum_kernel, dim3(1), dim3(256), 0, st, g, scratch, out, 0);
  return hipGetLastError();
}

// ---------------------------------------------------------------- K-GS-lex ---
// Exact lexicographic Gauss-Seidel (smoother.hpp:101-174) under a dependency
// schedule built on the host (host_setup.cpp: build_lex_schedule).  ONE
// workgroup walks the level window by window (BLOCK slots per window).  Inside
// a window every lane first gathers the u values that do not come from this
// window (old values and values finished by earlier windows), then the window
// is resolved in `win_depth+1` steps: a lane at dependency depth d sums its
// row in ascending column order, taking in-window producers from LDS.  Any
// execution that honours the dependencies and keeps each row's summation order
// reproduces the sequential sweep bit for bit.
//   MODE 0: SparseGaussSeidel update  (b - rsum)/diag, unchanged if diag == 0
//   MODE 1: AMG::Jacobi               (b - sigma)/aii  (aii = 0 if absent)
//   MODE 2: SOR  uk + omega*((b - s_less - s_greater)/aii - uk)
template <int BLOCK, int MAXE>
__global__ __launch_bounds__(BLOCK) void gs_lex_window(
    int64_t n_slots, int width, const int32_t* __restrict__ slot_row,
    const int16_t* __restrict__ slot_depth, const int32_t* __restrict__ win_depth,
    const int32_t* __restrict__ ecol, const double* __restrict__ eval,
    const int16_t* __restrict__ esrc, const double* __restrict__ b, double* u,
    int mode, double omega) {
  __shared__ double pub[BLOCK];
  const int lane = threadIdx.x;
  const int64_t n_win = n_slots / BLOCK;
  for (int64_t w = 0; w < n_win; ++w) {
    const int64_t slot = w * BLOCK + lane;
    const int row = slot_row[slot];
    const int depth = slot_depth[slot];
    const int wd = win_depth[w];
    // per entry: kind 0 = absent / diagonal, 1 = term of the (first) sum, 2 = term
    // of SOR's second sum (j > i, smoother.hpp:354-357); term = product that is
    // already known (operand outside this window) or v * (value published in LDS).
    // Everything is written branch-free (clamped addresses + selects) so that the
    // loads of a phase are issued back to back instead of one wait per entry.
    int sidx[MAXE];   // LDS slot of the in-window producer (0 when none)
    bool dep[MAXE];
    int kind[MAXE];
    double v[MAXE], term[MAXE];
    const bool live = row >= 0;
    const int rowc = live ? row : 0;
    const double bi = b[rowc];
    const double uk = u[rowc];
    double diag = 0.0;
    int32_t c[MAXE];
    int32_t sr[MAXE];
#pragma unroll
    for (int e = 0; e < MAXE; ++e) {
      const int ee = e < width ? e : 0;
      const int64_t at = (int64_t)ee * n_slots + slot;
      c[e] = ecol[at];
      v[e] = eval[at];
      sr[e] = esrc[at];
    }
    double ug[MAXE];
#pragma unroll
    for (int e = 0; e < MAXE; ++e) {
      const bool entry = live && e < width && c[e] >= 0;
      ug[e] = u[entry ? c[e] : 0];
    }
#pragma unroll
    for (int e = 0; e < MAXE; ++e) {
      const bool entry = live && e < width && c[e] >= 0;
      const bool isdiag = entry && c[e] == row;
      diag = isdiag ? v[e] : diag;
      const bool off = entry && !isdiag;
      dep[e] = off && sr[e] >= 0;
      sidx[e] = dep[e] ? sr[e] : 0;
      kind[e] = off ? ((mode == 2 && c[e] > row) ? 2 : 1) : 0;
      term[e] = v[e] * ug[e];  // operand final (earlier window) or old value
    }
    double unew = uk;
    for (int d = 0; d <= wd; ++d) {
      double pv[MAXE];
#pragma unroll
      for (int e = 0; e < MAXE; ++e) pv[e] = pub[sidx[e]];
      double s = 0.0, s2 = 0.0;
#pragma unroll
      for (int e = 0; e < MAXE; ++e) {
        const double t = dep[e] ? v[e] * pv[e] : term[e];
        s = (kind[e] == 1) ? s + t : s;
        s2 = (kind[e] == 2) ? s2 + t : s2;
      }
      double cand;
      if (mode == 0) cand = (diag == 0.0) ? uk : (bi - s) / diag;
      else if (mode == 1) cand = (bi - s) / diag;
      else cand = uk + omega * ((bi - s - s2) / diag - uk);
      unew = (live && depth == d) ? cand : unew;
      __syncthreads();       // everybody has read pub of the previous step
      pub[lane] = unew;      // final once depth <= d; earlier values are never consumed
      __syncthreads();
    }
    if (live) u[row] = unew;
    __threadfence_block();
    __syncthreads();
  }
}

template <int BLOCK>
static hipError_t launch_gs_lex_b(const LexDev& S, const double* b, double* u, int mode,
                                  double omega, hipStream_t st) {
#define AMG_LEX(M) hipLaunchKernelGGL((gs_lex_window<BLOCK, M>), dim3(1), dim3(BLOCK), 0, st, S.n_slots, \
                                      S.width, S.row, S.depth, S.win_depth, S.col, S.val, S.src, b, u, mode, omega)
  if (S.width <= 5) AMG_LEX(5);
  else if (S.width <= 7) AMG_LEX(7);
  else if (S.width <= 9) AMG_LEX(9);
  else if (S.width <= 16) AMG_LEX(16);
  else if (S.width <= 32) AMG_LEX(32);  // irregular coarse operators (strength-based coarsening, 3-D)
  else AMG_LEX(64);
#undef AMG_LEX
  return hipGetLastError();
}
hipError_t launch_gs_lex(const LexDev& S, const double* b, double* u, int mode, double omega,
                         hipStream_t st) {
  if (S.n_slots <= 0) return hipSuccess;
  if (S.width > 64) return hipErrorInvalidValue;
  switch (S.block) {
    case 64: return launch_gs_lex_b<64>(S, b, u, mode, omega, st);
    case 256: return launch_gs_lex_b<256>(S, b, u, mode, omega, st);
    case 1024: return launch_gs_lex_b<1024>(S, b, u, mode, omega, st);
  }
  return hipErrorInvalidValue;
}

static int g_scan_typed = 1;
static int g_scan_long = [] {  // chunks of more than 1024 rows (AMG_HIP_SCAN_LONG=0: the round-2 walk)
  const char* e = std::getenv("AMG_HIP_SCAN_LONG");
  return (e && *e == '0') ? 0 : 1;
}();
bool gs_scan_long_chunks_ok(const DictRef& D) { return g_scan_long && D.rtype && g_scan_typed && D.scan_new <= 4; }
void set_scan_typed(int on) { g_scan_typed = on ? 1 : 0; }
// --------------------------------------------------------------- K-GS-scan ---
// Lexicographic Gauss-Seidel at size (smoother.hpp:148-174).  On the reference's Galerkin
// levels row k of a forward sweep needs the NEW values of k-1 (the flat-index chain, SURVEY
// F9) and of rows at least g = m-1 back (the previous grid line); everything else is old.
// Inside a chunk of C <= g consecutive rows only the chain is unresolved, and it is a
// first-order linear recurrence
//     u_k = c_k + q_k u_{k-1},   c_k = (b_k - S_new - S_old) / a_kk,   q_k = -a_{k,k-1} / a_kk
// (SOR: c, q blended with omega and the old u_k) that a parallel affine scan solves in
// log C steps: (q, c) o (Q, C) = (q Q, c + q C).  ONE workgroup of 1024 threads walks the
// level chunk by chunk: S_old (terms of rows not yet swept) is formed one chunk ahead from
// global memory, S_new from an LDS ring of the last g + C new values, wave-level scan with
// DPP shuffles, wave totals combined through LDS.  Same sweep, different rounding order
// (|q| ~ 0.13-0.23: errors do not grow): agrees with the sequential sweep to ~1e-13, which
// is why the exact dependency-scheduled kernel stays the default on small problems and
// under opt.exact_gs.  The backward sweep is the same walk from the last row with the
// roles of lower and upper entries swapped.
//   mode 0: SparseGaussSeidel update (rows without diagonal keep their value)
//   mode 1: AMG::Jacobi (forward GS)      mode 2: SOR with omega
struct ScanEntry { double v; int32_t off; int32_t pad; };
// row structure of a dictionary-coded row: code words from the row type or the per-row codes
template <int WORDS>
__device__ __forceinline__ void scan_row_words(uint64_t (&cw)[2], int k, const uint64_t* __restrict__ codes,
                                               const uint8_t* __restrict__ rtype, const uint64_t* wtab) {
  cw[0] = cw[1] = ~(uint64_t)0;
  if (rtype) {
    const uint32_t ty = rtype[k];
#pragma unroll
    for (int w = 0; w < WORDS; ++w) cw[w] = wtab[ty * WORDS + w];
  } else {
#pragma unroll
    for (int w = 0; w < WORDS; ++w) cw[w] = codes[(int64_t)k * WORDS + w];
  }
}
__device__ __forceinline__ void scan_stage_tables(ScanEntry* tab, uint64_t* wtab, int words,
                                                  const uint8_t* rtype, const uint64_t* __restrict__ rwords,
                                                  const int32_t* __restrict__ doff,
                                                  const double* __restrict__ dval, int ntab) {
  const int t = threadIdx.x;
  if (t < 256) {
    ScanEntry e;
    e.v = t < ntab ? dval[t] : 0.0;
    e.off = t < ntab ? doff[t] : 0;
    e.pad = 0;
    tab[t] = e;
    if (rtype)
      for (int k = 0; k < words; ++k) wtab[t * words + k] = rwords[t * words + k];
  }
}
// Pre-pass, parallel over the whole level: the part of every row sum that a sweep takes from
// rows it has not reached yet (forward: columns above the diagonal, backward: below) -- old
// values, known before the sweep starts.  s_old[k] = sum in ascending column order.
template <int WORDS, int UN>
__global__ __launch_bounds__(256) void gs_scan_prep_kernel(
    int n, const uint64_t* __restrict__ codes, const uint8_t* __restrict__ rtype,
    const uint64_t* __restrict__ rwords, const int32_t* __restrict__ doff,
    const double* __restrict__ dval, int ntab, const double* __restrict__ u, int backward,
    double* __restrict__ s_old) {
  __shared__ ScanEntry tab[256];
  __shared__ uint64_t wtab[256 * WORDS];
  scan_stage_tables(tab, wtab, WORDS, rtype, rwords, doff, dval, ntab);
  __syncthreads();
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  uint64_t cw[2];
  scan_row_words<WORDS>(cw, k, codes, rtype, wtab);
  double uv[UN], vv[UN];
  bool side[UN];
#pragma unroll
  for (int e = 0; e < UN; ++e) {
    const uint32_t code = (uint32_t)(cw[e >> 3] >> (8 * (e & 7))) & 0xFFu;
    const ScanEntry en = tab[code == 0xFFu ? 0 : code];
    side[e] = code != 0xFFu && (backward ? en.off < 0 : en.off > 0);
    vv[e] = en.v;
    uv[e] = u[side[e] ? k + en.off : k];
  }
  double s = 0.0;
#pragma unroll
  for (int e = 0; e < UN; ++e) s = side[e] ? s + vv[e] * uv[e] : s;
  s_old[k] = s;
}

// wave-level inclusive scan of affine maps with DPP row shifts / broadcasts (no LDS crossbar
// round trips): after it lane i holds the composition of lanes 0..i
template <int CTRL, int ROWMASK>
__device__ __forceinline__ double dpp_f64(double ident, double v) {
  const int lo = __builtin_amdgcn_update_dpp(__double2loint(ident), __double2loint(v), CTRL, ROWMASK, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(__double2hiint(ident), __double2hiint(v), CTRL, ROWMASK, 0xF, false);
  return __hiloint2double(hi, lo);
}
template <int CTRL, int ROWMASK>
__device__ __forceinline__ void affine_step(double& Q, double& Cc) {
  const double Qp = dpp_f64<CTRL, ROWMASK>(1.0, Q), Cp = dpp_f64<CTRL, ROWMASK>(0.0, Cc);
  Cc = Cc + Q * Cp;   // (q, c) o (Qp, Cp): lanes without a source see the identity (1, 0)
  Q = Q * Qp;
}
__device__ __forceinline__ void affine_scan_wave(double& Q, double& Cc) {
  affine_step<0x111, 0xF>(Q, Cc);  // row_shr:1
  affine_step<0x112, 0xF>(Q, Cc);  // row_shr:2
  affine_step<0x114, 0xF>(Q, Cc);  // row_shr:4
  affine_step<0x118, 0xF>(Q, Cc);  // row_shr:8
  affine_step<0x142, 0xA>(Q, Cc);  // row_bcast:15 into rows 1 and 3
  affine_step<0x143, 0xC>(Q, Cc);  // row_bcast:31 into rows 2 and 3
}

template <int WORDS, int UN>
__global__ __launch_bounds__(1024) void gs_scan_kernel(
    int n, const uint64_t* __restrict__ codes, const uint8_t* __restrict__ rtype,
    const uint64_t* __restrict__ rwords, const int32_t* __restrict__ doff,
    const double* __restrict__ dval, int ntab, const double* __restrict__ b, double* u,
    const double* __restrict__ s_old, int backward, int mode, double omega, int C, int ringmask) {
  extern __shared__ double ring[];           // new values of the last rows, by row & ringmask
  __shared__ ScanEntry tab[256];
  __shared__ uint64_t wtab[256 * WORDS];
  __shared__ double totQ[16], totC[16], carry_in[16];
  __shared__ double last_u;                  // new value of the row before this chunk
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  scan_stage_tables(tab, wtab, WORDS, rtype, rwords, doff, dval, ntab);
  for (int i = t; i <= ringmask; i += (int)blockDim.x) ring[i] = 0.0;
  if (t == 0) last_u = 0.0;
  __syncthreads();
  const int nchunks = (n + C - 1) / C;
  const int chain = backward ? 1 : -1;       // offset of the chained neighbour
  // operands of one row, fetched two chunks ahead
  // (only global loads here, nothing that depends on them: the type -> code word lookup
  // happens when the row is used, two chunks later)
  struct Row {
    uint64_t cw[2];
    uint32_t ty;
    double bk, uk, so;
    int k;
    bool live;
  };
  auto fetch = [&](int chunk, Row& r) {
    const int idx = chunk * C + t;
    r.live = chunk < nchunks && t < C && idx < n;
    r.k = backward ? n - 1 - idx : idx;
    r.cw[0] = r.cw[1] = ~(uint64_t)0;
    r.ty = 255;
    r.bk = r.uk = r.so = 0.0;
    if (!r.live) return;
    if (rtype) {
      r.ty = rtype[r.k];
    } else {
#pragma unroll
      for (int w = 0; w < WORDS; ++w) r.cw[w] = codes[(int64_t)r.k * WORDS + w];
    }
    r.bk = b[r.k];
    r.uk = u[r.k];
    r.so = s_old[r.k];
  };
  // waves beyond the chunk length only take part in the barriers
  const bool active = wave * 64 < C;
  const int nwaves = (C + 63) >> 6;
  Row cur, nx1, nx2;
  cur.live = nx1.live = nx2.live = false;
  if (active) {
    fetch(0, cur);
    fetch(1, nx1);
  }
  for (int chunk = 0; chunk < nchunks; ++chunk) {
    double Q = 1.0, Cc = 0.0;
    if (active) {
      fetch(chunk + 2, nx2);  // in flight during two scans
      // (q, c) of this row from the new values of earlier chunks
      double q = 0.0, c = 0.0;
      if (cur.live) {
        if (rtype) {
#pragma unroll
          for (int w = 0; w < WORDS; ++w) cur.cw[w] = wtab[cur.ty * WORDS + w];
        }
        double s_new = 0.0, diag = 0.0, achain = 0.0;
#pragma unroll
        for (int e = 0; e < UN; ++e) {
          const uint32_t code = (uint32_t)(cur.cw[e >> 3] >> (8 * (e & 7))) & 0xFFu;
          const ScanEntry en = tab[code == 0xFFu ? 0 : code];
          const bool used = code != 0xFFu;
          const bool isdiag = used && en.off == 0;
          const bool ischain = used && en.off == chain;
          const bool new_side = used && !ischain && (backward ? en.off > 0 : en.off < 0);
          diag = isdiag ? en.v : diag;
          achain = ischain ? en.v : achain;
          const double rv = ring[(cur.k + (new_side ? en.off : 0)) & ringmask];
          s_new = new_side ? s_new + en.v * rv : s_new;
        }
        const double rsum = s_new + cur.so;
        if (mode == 0 && diag == 0.0) {       // smoother.hpp:134-137: row left alone
          c = cur.uk;
          q = 0.0;
        } else {
          const double g = (cur.bk - rsum) / diag;
          const double qq = -achain / diag;
          if (mode == 2) {                    // u_k + omega (g - u_k), smoother.hpp:360-362
            c = cur.uk + omega * (g - cur.uk);
            q = omega * qq;
          } else {
            c = g;
            q = qq;
          }
        }
      }
      // inclusive affine scan inside the wave: (Q, Cc) maps the value before the wave's
      // first row to this row's value
      Q = q;
      Cc = c;
      affine_scan_wave(Q, Cc);
      if (lane == 63) {
        totQ[wave] = Q;
        totC[wave] = Cc;
      }
    }
    lds_barrier();
    // second level: wave 0 turns the wave totals into the value BEFORE each wave's first row
    if (wave == 0) {
      double tq = lane < nwaves ? totQ[lane & 15] : 1.0, tc = lane < nwaves ? totC[lane & 15] : 0.0;
      affine_scan_wave(tq, tc);
      const double after = tc + tq * last_u;     // value of wave `lane`'s last row
      if (lane < 15) carry_in[lane + 1] = after;
      if (lane == 0) carry_in[0] = last_u;
    }
    lds_barrier();
    if (active) {
      const double unew = Cc + Q * carry_in[wave];
      if (cur.live) {
        ring[cur.k & ringmask] = unew;
        u[cur.k] = unew;
      }
      const int last_t = (chunk * C + C <= n ? C : n - chunk * C) - 1;
      if (t == last_t) last_u = unew;
    }
    lds_barrier();                             // ring and last_u are ready for the next chunk
    cur = nx1;
    nx1 = nx2;
  }
}

// ---- row-typed matrices: everything that does not depend on new values moves to the pre-pass
// The chain coefficient, the diagonal and the weights of the new-side entries are properties
// of the row TYPE.  The pre-pass therefore leaves ONE number per row,
//   P_k = (b_k - s_old_k) / a_kk          (SOR: u_k + omega (that - u_k); rows that SpGS leaves
//                                          alone: u_k, with all weights 0),
// and the serial kernel evaluates  c_k = P_k - sum_e w_e u_new[k + off_e],  q_k = Q  with
// w_e = a_e / a_kk (x omega), Q = -a_chain / a_kk (x omega) from a per-type LDS table: no code
// words, no division and at most SCAN_NEW ring reads on the serial path.
__device__ __forceinline__ double readlane_f64(double v, int lane);  // K-Band section below
constexpr int SCAN_NEW = 4;  // new-side entries other than the chain, per row type (2-D: 3)
// per-type table as three LDS arrays: tq[256], tw[256 * SCAN_NEW], toff[256 * SCAN_NEW];
// thread t < 256 builds the entry of type t from its code words (type 255 / unused: zeros)
template <int WORDS, int UN>
__device__ __forceinline__ void scan_build_types(double* tq, double* tw, int32_t* toff,
                                                 const ScanEntry* tab, const uint64_t* wtab,
                                                 int backward, int mode, double omega) {
  const int t = threadIdx.x;
  if (t >= 256) return;
  const int chain = backward ? 1 : -1;
  double diag = 0.0, achain = 0.0;
  for (int e = 0; e < UN; ++e) {
    const uint32_t code = (uint32_t)(wtab[t * WORDS + (e >> 3)] >> (8 * (e & 7))) & 0xFFu;
    if (code != 0xFFu) {
      const ScanEntry en = tab[code];
      if (en.off == 0) diag = en.v;
      if (en.off == chain) achain = en.v;
    }
  }
  const bool frozen = mode == 0 && diag == 0.0;  // smoother.hpp:134-137
  const double sc = mode == 2 ? omega : 1.0;
  for (int e = 0; e < SCAN_NEW; ++e) {
    tw[t * SCAN_NEW + e] = 0.0;
    toff[t * SCAN_NEW + e] = 0;
  }
  tq[t] = frozen ? 0.0 : sc * (-achain / diag);
  int nn = 0;
  for (int e = 0; e < UN; ++e) {
    const uint32_t code = (uint32_t)(wtab[t * WORDS + (e >> 3)] >> (8 * (e & 7))) & 0xFFu;
    if (code == 0xFFu || frozen) continue;
    const ScanEntry en = tab[code];
    const bool new_side = en.off != chain && (backward ? en.off > 0 : en.off < 0);
    if (new_side && nn < SCAN_NEW) {
      tw[t * SCAN_NEW + nn] = sc * (en.v / diag);
      toff[t * SCAN_NEW + nn] = en.off;
      ++nn;
    }
  }
}
template <int WORDS, int UN>
__global__ __launch_bounds__(256) void gs_scan_prep_typed_kernel(
    int n, const uint8_t* __restrict__ rtype, const uint64_t* __restrict__ rwords,
    const int32_t* __restrict__ doff, const double* __restrict__ dval, int ntab,
    const double* __restrict__ b, const double* __restrict__ u, int backward, int mode, double omega,
    double* __restrict__ P) {
  __shared__ ScanEntry tab[256];
  __shared__ uint64_t wtab[256 * WORDS];
  scan_stage_tables(tab, wtab, WORDS, rtype, rwords, doff, dval, ntab);
  __syncthreads();
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  uint64_t cw[2];
  scan_row_words<WORDS>(cw, k, rwords, rtype, wtab);  // (codes unused: the matrix is row-typed)
  double uv[UN], vv[UN];
  bool side[UN];
  double diag = 0.0;
#pragma unroll
  for (int e = 0; e < UN; ++e) {
    const uint32_t code = (uint32_t)(cw[e >> 3] >> (8 * (e & 7))) & 0xFFu;
    const ScanEntry en = tab[code == 0xFFu ? 0 : code];
    side[e] = code != 0xFFu && (backward ? en.off < 0 : en.off > 0);
    diag = (code != 0xFFu && en.off == 0) ? en.v : diag;
    vv[e] = en.v;
    uv[e] = u[side[e] ? k + en.off : k];
  }
  double s = 0.0;
#pragma unroll
  for (int e = 0; e < UN; ++e) s = side[e] ? s + vv[e] * uv[e] : s;
  const double uk = u[k];
  double p;
  if (mode == 0 && diag == 0.0) {
    p = uk;
  } else {
    const double g = (b[k] - s) / diag;
    p = mode == 2 ? uk + omega * (g - uk) : g;
  }
  P[k] = p;
}
template <int WORDS, int UN>
__global__ __launch_bounds__(1024) void gs_scan_typed_kernel(
    int n, const uint8_t* __restrict__ rtype, const uint64_t* __restrict__ rwords,
    const int32_t* __restrict__ doff, const double* __restrict__ dval, int ntab, double* u,
    const double* __restrict__ P, int backward, int mode, double omega, int C, int ringmask) {
  extern __shared__ double ring[];           // new values of the last rows, by row & ringmask
  __shared__ ScanEntry tab[256];
  __shared__ uint64_t wtab[256 * WORDS];
  __shared__ double tq[256];
  __shared__ double tw[256 * SCAN_NEW];
  __shared__ int32_t toff[256 * SCAN_NEW];
  __shared__ double totQ[16], totC[16], carry_in[16];
  __shared__ double last_u;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  scan_stage_tables(tab, wtab, WORDS, rtype, rwords, doff, dval, ntab);
  for (int i = t; i <= ringmask; i += (int)blockDim.x) ring[i] = 0.0;
  if (t == 0) last_u = 0.0;
  __syncthreads();
  scan_build_types<WORDS, UN>(tq, tw, toff, tab, wtab, backward, mode, omega);
  __syncthreads();
  const int nchunks = (n + C - 1) / C;
  struct Row {
    double p;
    uint32_t ty;
    int k;
    bool live;
  };
  auto fetch = [&](int chunk, Row& r) {
    const int idx = chunk * C + t;
    r.live = chunk < nchunks && t < C && idx < n;
    r.k = backward ? n - 1 - idx : idx;
    r.ty = 255;
    r.p = 0.0;
    if (!r.live) return;
    r.ty = rtype[r.k];
    r.p = P[r.k];
  };
  const bool active = wave * 64 < C;
  const int nwaves = (C + 63) >> 6;
  Row cur, nx1, nx2;
  cur.live = nx1.live = nx2.live = false;
  if (active) {
    fetch(0, cur);
    fetch(1, nx1);
  }
  if (nwaves == 1) {
    // A chunk of at most 64 rows (the deep levels: short grid lines) is ONE wave's scan: no
    // cross-wave combine, no barrier -- the wave's LDS accesses keep their order -- and the
    // carry travels in a register.  Same products and sums as the general path below.
    if (wave != 0) return;
    double carry = 0.0;  // wave-uniform: the last new value of the previous chunk
    for (int chunk = 0; chunk < nchunks; ++chunk) {
      fetch(chunk + 2, nx2);
      double q = 0.0, c = 0.0;
      if (cur.live) {
        const int tb = (int)cur.ty * SCAN_NEW;
        double rv[SCAN_NEW], wv[SCAN_NEW];
#pragma unroll
        for (int e = 0; e < SCAN_NEW; ++e) {
          wv[e] = tw[tb + e];
          rv[e] = ring[(cur.k + toff[tb + e]) & ringmask];
        }
        c = cur.p;
#pragma unroll
        for (int e = 0; e < SCAN_NEW; ++e) c -= wv[e] * rv[e];
        q = tq[cur.ty];
      }
      double Q = q, Cc = c;
      affine_scan_wave(Q, Cc);
      const double unew = Cc + Q * carry;
      if (cur.live) {
        ring[cur.k & ringmask] = unew;
        u[cur.k] = unew;
      }
      const int last_t = (chunk * C + C <= n ? C : n - chunk * C) - 1;
      carry = readlane_f64(unew, last_t);
      cur = nx1;
      nx1 = nx2;
    }
    return;
  }
  uint32_t cty = 0xFFFFFFFFu;  // row type whose weights the lane holds
  double cwv[SCAN_NEW], cqv = 0.0;
  int32_t cof[SCAN_NEW];
#pragma unroll
  for (int e = 0; e < SCAN_NEW; ++e) {
    cwv[e] = 0.0;
    cof[e] = 0;
  }
  for (int chunk = 0; chunk < nchunks; ++chunk) {
    double Q = 1.0, Cc = 0.0;
    if (active) {
      fetch(chunk + 2, nx2);  // in flight during two scans
      double q = 0.0, c = 0.0;
      // the weights of the lane's row type stay in registers from chunk to chunk: a lane walks
      // down one grid column, whose rows share a type except at the first and last lines, so the
      // nine table reads per row (of thirteen LDS reads) are skipped while no lane of the wave
      // changes type -- one workgroup's LDS instruction rate is what bounds this kernel
      if (__builtin_amdgcn_ballot_w64(cur.ty != cty) != 0) {
        const int tb = (int)cur.ty * SCAN_NEW;
#pragma unroll
        for (int e = 0; e < SCAN_NEW; ++e) {
          cwv[e] = tw[tb + e];
          cof[e] = toff[tb + e];
        }
        cqv = tq[cur.ty];
        cty = cur.ty;
      }
      if (cur.live) {
        double rv[SCAN_NEW];
#pragma unroll
        for (int e = 0; e < SCAN_NEW; ++e) rv[e] = ring[(cur.k + cof[e]) & ringmask];
        c = cur.p;
#pragma unroll
        for (int e = 0; e < SCAN_NEW; ++e) c -= cwv[e] * rv[e];   // unused slots: weight 0
        q = cqv;
      }
      Q = q;
      Cc = c;
      affine_scan_wave(Q, Cc);
      if (lane == 63) {
        totQ[wave] = Q;
        totC[wave] = Cc;
      }
    }
    lds_barrier();
    if (wave == 0) {
      double tq = lane < nwaves ? totQ[lane & 15] : 1.0, tc = lane < nwaves ? totC[lane & 15] : 0.0;
      affine_scan_wave(tq, tc);
      const double after = tc + tq * last_u;
      if (lane < 15) carry_in[lane + 1] = after;
      if (lane == 0) carry_in[0] = last_u;
    }
    lds_barrier();
    if (active) {
      const double unew = Cc + Q * carry_in[wave];
      if (cur.live) {
        ring[cur.k & ringmask] = unew;
        u[cur.k] = unew;
      }
      const int last_t = (chunk * C + C <= n ? C : n - chunk * C) - 1;
      if (t == last_t) last_u = unew;
    }
    lds_barrier();
    cur = nx1;
    nx1 = nx2;
  }
}

// The same walk with R = 2 or 4 CONSECUTIVE rows per thread, for chunks of more than 1024 rows (grid
// lines of 2048 / 4096 and more: the finest levels of the big grids).  A chunk may be as long as
// the distance to the previous grid line, and the serial walk pays per CHUNK (three barriers, two
// scan levels), so a 4096-wide level takes a quarter of the chunks.  A thread folds its R affine
// maps into one, the wave and workgroup scans run on the folded maps as before, and the thread
// then walks its rows from the value before its block (the exclusive prefix: the inclusive result
// of the lane below, through one cross-lane shift).  Same recurrence; the association of the
// products differs from the one-row kernel (as that one's differs from the sequential sweep):
// 1e-13 class.
template <int WORDS, int UN, int R>
__global__ __launch_bounds__(1024) void gs_scan_typed_rows_kernel(
    int n, const uint8_t* __restrict__ rtype, const uint64_t* __restrict__ rwords,
    const int32_t* __restrict__ doff, const double* __restrict__ dval, int ntab, double* u,
    const double* __restrict__ P, int backward, int mode, double omega, int C, int ringmask) {
  extern __shared__ double ring[];
  __shared__ ScanEntry tab[256];
  __shared__ uint64_t wtab[256 * WORDS];
  __shared__ double tq[256];
  __shared__ double tw[256 * SCAN_NEW];
  __shared__ int32_t toff[256 * SCAN_NEW];
  __shared__ double totQ[16], totC[16], carry_in[16];
  __shared__ double last_u;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  scan_stage_tables(tab, wtab, WORDS, rtype, rwords, doff, dval, ntab);
  for (int i = t; i <= ringmask; i += (int)blockDim.x) ring[i] = 0.0;
  if (t == 0) last_u = 0.0;
  __syncthreads();
  scan_build_types<WORDS, UN>(tq, tw, toff, tab, wtab, backward, mode, omega);
  __syncthreads();
  const int nchunks = (n + C - 1) / C;
  struct Row {
    double p;
    uint32_t ty;
    int k;
    bool live;
  };
  auto fetch = [&](int chunk, Row (&rw)[R]) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int j = t * R + r;
      const int idx = chunk * C + j;
      rw[r].live = chunk < nchunks && j < C && idx < n;
      rw[r].k = backward ? n - 1 - idx : idx;
      rw[r].ty = 255;
      rw[r].p = 0.0;
      if (rw[r].live) {
        rw[r].ty = rtype[rw[r].k];
        rw[r].p = P[rw[r].k];
      }
    }
  };
  const int nwaves = ((C + R - 1) / R + 63) >> 6;
  const bool active = wave < nwaves;
  Row cur[R], nx1[R], nx2[R];
#pragma unroll
  for (int r = 0; r < R; ++r) cur[r].live = nx1[r].live = nx2[r].live = false;
  if (active) {
    fetch(0, cur);
    fetch(1, nx1);
  }
  for (int chunk = 0; chunk < nchunks; ++chunk) {
    double q[R], c[R];
    double Q = 1.0, Cc = 0.0;
    if (active) {
      fetch(chunk + 2, nx2);  // in flight during two scans
#pragma unroll
      for (int r = 0; r < R; ++r) {
        q[r] = 0.0;
        c[r] = 0.0;
        // (the one-row kernel keeps the weights of a lane's row type in registers from chunk to
        // chunk; with R rows per lane that costs more registers than it saves LDS reads: 4096^2
        // 221 -> 241 ms per cycle, not kept here)
        if (cur[r].live) {
          const int tb = (int)cur[r].ty * SCAN_NEW;
          double rv[SCAN_NEW], wv[SCAN_NEW];
#pragma unroll
          for (int e = 0; e < SCAN_NEW; ++e) {
            wv[e] = tw[tb + e];
            rv[e] = ring[(cur[r].k + toff[tb + e]) & ringmask];
          }
          double cc = cur[r].p;
#pragma unroll
          for (int e = 0; e < SCAN_NEW; ++e) cc -= wv[e] * rv[e];   // unused slots: weight 0
          c[r] = cc;
          q[r] = tq[cur[r].ty];
        }
      }
      // the thread's R maps folded into one: (q_r, c_r) o (Q, Cc) = (q_r Q, c_r + q_r Cc)
      Q = q[0];
      Cc = c[0];
#pragma unroll
      for (int r = 1; r < R; ++r) {
        Cc = c[r] + q[r] * Cc;
        Q = q[r] * Q;
      }
      affine_scan_wave(Q, Cc);
      if (lane == 63) {
        totQ[wave] = Q;
        totC[wave] = Cc;
      }
    }
    lds_barrier();
    if (wave == 0) {
      double sq = lane < nwaves ? totQ[lane & 15] : 1.0, sc = lane < nwaves ? totC[lane & 15] : 0.0;
      affine_scan_wave(sq, sc);
      const double after = sc + sq * last_u;
      if (lane < 15) carry_in[lane + 1] = after;
      if (lane == 0) carry_in[0] = last_u;
    }
    lds_barrier();
    if (active) {
      // value before this thread's block: the inclusive result of the lane below applied to the
      // wave's carry (lane 0: the carry itself)
      double Qp = __shfl_up(Q, 1), Cp = __shfl_up(Cc, 1);
      if (lane == 0) {
        Qp = 1.0;
        Cp = 0.0;
      }
      double v = Cp + Qp * carry_in[wave];
      const int len = (chunk * C + C <= n ? C : n - chunk * C);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        v = c[r] + q[r] * v;
        if (cur[r].live) {
          ring[cur[r].k & ringmask] = v;
          u[cur[r].k] = v;
        }
        if (t * R + r == len - 1) last_u = v;
      }
    }
    lds_barrier();                             // ring and last_u are ready for the next chunk
#pragma unroll
    for (int r = 0; r < R; ++r) {
      cur[r] = nx1[r];
      nx1[r] = nx2[r];
    }
  }
}
constexpr int GS_SCAN_MAX_CHUNK = 4096;
int gs_scan_max_chunk() { return GS_SCAN_MAX_CHUNK; }

template <int WORDS, int UN>
static hipError_t launch_gs_scan_wu(int64_t n, const DictRef& D, const double* b, double* u,
                                    double* s_old, int backward, int mode, double omega, int C,
                                    int ring, hipStream_t st) {
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&gs_scan_kernel<WORDS, UN>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 131072);
    attr_set = true;
  }
  if (D.rtype && g_scan_typed && D.scan_new <= SCAN_NEW) {
    static bool attr2 = false;
    if (!attr2) {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&gs_scan_typed_kernel<WORDS, UN>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, 131072);
      attr2 = true;
    }
    hipLaunchKernelGGL((gs_scan_prep_typed_kernel<WORDS, UN>), dim3((unsigned)((n + 255) / 256)), dim3(256),
                       0, st, (int)n, D.rtype, D.rwords, D.doff, D.dval, D.ntab, b, u, backward, mode, omega,
                       s_old);
    if (C > 1024) {  // long grid lines: 2 or 4 consecutive rows per thread
      static bool attr3 = false;
      if (!attr3) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&gs_scan_typed_rows_kernel<WORDS, UN, 2>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 131072);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&gs_scan_typed_rows_kernel<WORDS, UN, 4>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 131072);
        attr3 = true;
      }
      if (C <= 2048)
        hipLaunchKernelGGL((gs_scan_typed_rows_kernel<WORDS, UN, 2>), dim3(1), dim3(1024), (size_t)ring * 8, st,
                           (int)n, D.rtype, D.rwords, D.doff, D.dval, D.ntab, u, s_old, backward, mode, omega, C,
                           ring - 1);
      else
        hipLaunchKernelGGL((gs_scan_typed_rows_kernel<WORDS, UN, 4>), dim3(1), dim3(1024), (size_t)ring * 8, st,
                           (int)n, D.rtype, D.rwords, D.doff, D.dval, D.ntab, u, s_old, backward, mode, omega, C,
                           ring - 1);
      return hipGetLastError();
    }
    // as many waves as the chunk has rows (at least the four that stage the tables): the three
    // barriers per chunk cost what the waves they hold up cost, and a deep level's chunk is short
    const int nt = std::max(256, (C + 63) / 64 * 64);
    hipLaunchKernelGGL((gs_scan_typed_kernel<WORDS, UN>), dim3(1), dim3(nt), (size_t)ring * 8, st, (int)n,
                       D.rtype, D.rwords, D.doff, D.dval, D.ntab, u, s_old, backward, mode, omega, C,
                       ring - 1);
    return hipGetLastError();
  }
  if (C > 1024) return hipErrorInvalidValue;  // only the row-typed form walks long chunks
  hipLaunchKernelGGL((gs_scan_prep_kernel<WORDS, UN>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                     (int)n, D.codes, D.rtype, D.rwords, D.doff, D.dval, D.ntab, u, backward, s_old);
  const int nt = std::max(256, (C + 63) / 64 * 64);
  hipLaunchKernelGGL((gs_scan_kernel<WORDS, UN>), dim3(1), dim3(nt), (size_t)ring * 8, st, (int)n,
                     D.codes, D.rtype, D.rwords, D.doff, D.dval, D.ntab, b, u, s_old, backward, mode,
                     omega, C, ring - 1);
  return hipGetLastError();
}
// C: rows per chunk (<= the distance of the nearest non-chain dependency; <= 1024, or <= 4096 on a
// row-typed matrix with at most SCAN_NEW new-side entries per row: gs_scan_long_chunks_ok);
// ring: power of two >= largest dependency distance + C + 1, at most 16384 doubles
hipError_t launch_gs_scan(int64_t n, const DictRef& D, const double* b, double* u, double* s_old,
                          bool backward, int mode, double omega, int C, int ring, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (!dict_args_ok(n, D.words, D.wmax, D.ntab) || C < 1 || C > GS_SCAN_MAX_CHUNK || ring < 2 || ring > 16384 ||
      (ring & (ring - 1)) || !s_old)
    return hipErrorInvalidValue;
  hipError_t r = hipSuccess;
  (void)dict_dispatch_wu(D.words, D.wmax, [&](auto W, auto U) {
    r = launch_gs_scan_wu<decltype(W)::value, decltype(U)::value>(n, D, b, u, s_old, backward ? 1 : 0,
                                                                  mode, omega, C, ring, st);
  });
  return r;
}

// ------------------------------------------------------- K-Halo (in-graph comm) ---
// Neighbour exchange as ONE graph-capturable kernel: the host-driven version
// (hipMemcpyAsync + hipStreamWrite/WaitValue32, solver.cpp) costs ~3 us of host
// time per stream operation and those operations cannot be captured in a hipGraph.
// Protocol per channel and direction, words in the RECEIVER's arena, values 0/1:
//   DATA  set to 1 by the sender after its boundary values landed in the
//         receiver's halo slots; reset to 0 by the receiver when it has seen it;
//   FREE  set to 1 by the receiver (halo_ack_kernel) once the kernel that read the
//         halo is done; reset to 0 by the sender before it overwrites the slots.
// One workgroup: lane 0 waits for FREE, all lanes copy (stores to the peer's
// hipIpc-mapped memory), system fence, lane 0 publishes DATA and waits for its
// own.  All flag accesses are system-scope atomics; every spin is bounded
// (~2 s of wall clock) and reports through `timeout`.
__device__ __forceinline__ bool spin_until_one(uint32_t* w, uint32_t* timeout) {
  const unsigned long long t0 = wall_clock64();
  while (__hip_atomic_load(w, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) != 1u) {
    if (wall_clock64() - t0 > 200000000ull) {  // 100 MHz constant clock
      __hip_atomic_store(timeout, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      return false;
    }
    __builtin_amdgcn_s_sleep(8);
  }
  __hip_atomic_store(w, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  return true;
}

__global__ __launch_bounds__(256) void halo_exchange_kernel(HaloArgs a) {
  const int t = threadIdx.x;
  if (t == 0) {
    if (a.cnt_prev > 0) spin_until_one(a.my_free_from_prev, a.timeout);
    if (a.cnt_next > 0) spin_until_one(a.my_free_from_next, a.timeout);
  }
  __syncthreads();
  for (int64_t i = t; i < a.cnt_prev; i += 256)
    __builtin_nontemporal_store(a.src_prev[i], a.dst_prev + i);
  for (int64_t i = t; i < a.cnt_next; i += 256)
    __builtin_nontemporal_store(a.src_next[i], a.dst_next + i);
  __threadfence_system();
  __syncthreads();
  if (t == 0) {
    if (a.cnt_prev > 0)
      __hip_atomic_store(a.data_at_prev, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    if (a.cnt_next > 0)
      __hip_atomic_store(a.data_at_next, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    if (a.recv_prev) spin_until_one(a.my_data_from_prev, a.timeout);
    if (a.recv_next) spin_until_one(a.my_data_from_next, a.timeout);
    __threadfence_system();
  }
}
__global__ void halo_ack_kernel(uint32_t* free_at_prev, uint32_t* free_at_next) {
  if (threadIdx.x == 0) {
    if (free_at_prev) __hip_atomic_store(free_at_prev, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    if (free_at_next) __hip_atomic_store(free_at_next, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}
// Large halos (3-D: one x-y plane, MBs): same protocol split over three launches so
// that the copy can use many workgroups.
__global__ void halo_wait_free_kernel(HaloArgs a) {
  if (threadIdx.x == 0) {
    if (a.cnt_prev > 0) spin_until_one(a.my_free_from_prev, a.timeout);
    if (a.cnt_next > 0) spin_until_one(a.my_free_from_next, a.timeout);
  }
}
__global__ __launch_bounds__(256) void halo_copy_kernel(HaloArgs a) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x, nt = (int64_t)gridDim.x * 256;
  for (int64_t i = t; i < a.cnt_prev; i += nt) __builtin_nontemporal_store(a.src_prev[i], a.dst_prev + i);
  for (int64_t i = t; i < a.cnt_next; i += nt) __builtin_nontemporal_store(a.src_next[i], a.dst_next + i);
  __threadfence_system();
}
__global__ void halo_publish_wait_kernel(HaloArgs a) {
  if (threadIdx.x == 0) {
    if (a.cnt_prev > 0)
      __hip_atomic_store(a.data_at_prev, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    if (a.cnt_next > 0)
      __hip_atomic_store(a.data_at_next, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    if (a.recv_prev) spin_until_one(a.my_data_from_prev, a.timeout);
    if (a.recv_next) spin_until_one(a.my_data_from_next, a.timeout);
    __threadfence_system();
  }
}
hipError_t launch_halo_exchange(const HaloArgs& a, hipStream_t st) {
  const int64_t big = a.cnt_prev > a.cnt_next ? a.cnt_prev : a.cnt_next;
  if (big <= 16384) {
    hipLaunchKernelGGL(halo_exchange_kernel, dim3(1), dim3(256), 0, st, a);
  } else {
    int64_t g = (big + 2047) / 2048;
    if (g > 256) g = 256;
    hipLaunchKernelGGL(halo_wait_free_kernel, dim3(1), dim3(64), 0, st, a);
    hipLaunchKernelGGL(halo_copy_kernel, dim3((unsigned)g), dim3(256), 0, st, a);
    hipLaunchKernelGGL(halo_publish_wait_kernel, dim3(1), dim3(64), 0, st, a);
  }
  return hipGetLastError();
}
hipError_t launch_halo_ack(uint32_t* free_at_prev, uint32_t* free_at_next, hipStream_t st) {
  if (!free_at_prev && !free_at_next) return hipSuccess;
  hipLaunchKernelGGL(halo_ack_kernel, dim3(1), dim3(64), 0, st, free_at_prev, free_at_next);
  return hipGetLastError();
}

// All-gather of the agglomeration level's right-hand side by direct pushes:
// rank r copies its slice into every rank's full vector at offset `off` (its own
// included).  k1: wait until every destination released the slot (FREE); k2: copy;
// k3: publish DATA everywhere and wait for everybody's DATA.
__global__ void gather_wait_free_kernel(GatherArgs a) {
  const int g = threadIdx.x;
  if (g < a.world && g != a.rank) spin_until_one(a.my_free_from + g, a.timeout);
}
__global__ __launch_bounds__(256) void gather_copy_kernel(GatherArgs a) {
  const int g = blockIdx.y;
  double* dst = a.dst[g] + a.off;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.cnt; i += (int64_t)gridDim.x * 256)
    dst[i] = a.src[i];
  __threadfence_system();
}
__global__ void gather_publish_wait_kernel(GatherArgs a) {
  const int g = threadIdx.x;
  if (g < a.world && g != a.rank) {
    __hip_atomic_store(a.data_at[g], 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    spin_until_one(a.my_data_from + g, a.timeout);
    __threadfence_system();
  }
}
__global__ void gather_ack_kernel(GatherArgs a) {
  const int g = threadIdx.x;
  if (g < a.world && g != a.rank)
    __hip_atomic_store(a.free_at[g], 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
hipError_t launch_gather(const GatherArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(gather_wait_free_kernel, dim3(1), dim3(64), 0, st, a);
  int64_t gx = (a.cnt + 255) / 256;
  if (gx > 64) gx = 64;
  if (gx < 1) gx = 1;
  hipLaunchKernelGGL(gather_copy_kernel, dim3((unsigned)gx, (unsigned)a.world), dim3(256), 0, st, a);
  hipLaunchKernelGGL(gather_publish_wait_kernel, dim3(1), dim3(64), 0, st, a);
  return hipGetLastError();
}
hipError_t launch_gather_ack(const GatherArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(gather_ack_kernel, dim3(1), dim3(64), 0, st, a);
  return hipGetLastError();
}

// ------------------------------------------------------------------ K-Band ---
// x = A^-1 f with A = L D L^T banded (half-bandwidth w <= 63), ONE wave -- the
// substitution is a serial chain, so the design goal is the fewest instructions
// per step.  M = power of two > w lanes take part; lane l keeps the running
// right-hand side of the rows == l (mod M) in a register.  Forward step s: y_s
// is complete in lane s%M -> v_readlane broadcast -> every lane subtracts its
// pre-scheduled L entry times y_s (one multiply, one subtract, no FMA: the
// updates reach a row in ascending s, the order of a row-oriented substitution).
// The host lays L out per (step, lane) (host_setup.cpp: band_schedule) so a
// step's operands are ONE coalesced load with an immediate offset, fetched a
// whole 32-step chunk ahead.  Then z = y / D (IEEE divide) and the mirrored
// backward pass (row i lives in lane (n-1-i) % M).
__device__ __forceinline__ double readlane_f64(double v, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}
// v_writelane_b32 has no clang builtin on this toolchain.  dst[lane] = uniform
// value; `lane` is wave-uniform.  (SALU-written lane select, SGPR data operand:
// no software wait states needed on gfx9-family for this pair.)
template <int LANE>  // immediate lane select: an SGPR one would be a 2nd constant-bus read
__device__ __forceinline__ void writelane_f64(double& dst, double uniform_v) {
  int lo = __double2loint(dst), hi = __double2hiint(dst);
  const int ulo = __builtin_amdgcn_readfirstlane(__double2loint(uniform_v));
  const int uhi = __builtin_amdgcn_readfirstlane(__double2hiint(uniform_v));
  asm volatile("v_writelane_b32 %0, %2, %4\n\tv_writelane_b32 %1, %3, %4"
               : "+v"(lo), "+v"(hi)
               : "s"(ulo), "s"(uhi), "n"(LANE));
  dst = __hiloint2double(hi, lo);
}

constexpr int BAND_CH = 32;  // steps per register-prefetched chunk

struct BandChunk {
  double lc[BAND_CH];  // lane l < M: its L operand for each of the 32 steps
  double nx;           // lane i < 32: right-hand side of the row picked up after step i
};

// FWD: step s handles row s; else row n-1-s.  The schedule is zero-padded to a
// multiple of 64 steps (+64), so there are no bounds checks on it.
template <int M, bool FWD>
__device__ __forceinline__ void band_load(BandChunk& c, int64_t s0, int64_t n, int lane,
                                          const double* __restrict__ sched,
                                          const double* __restrict__ rhs) {
  if (lane < M) {
    const double* p = sched + s0 * M + lane;
#pragma unroll
    for (int i = 0; i < BAND_CH; ++i) c.lc[i] = p[i * M];
  } else {
#pragma unroll
    for (int i = 0; i < BAND_CH; ++i) c.lc[i] = 0.0;
  }
  // after step s0+i its owner lane picks up row s0+i+M; rows past the end read
  // as 0.0 so that the padded steps broadcast 0.0, never garbage
  const int64_t s2 = s0 + lane + M;
  const bool ok = lane < BAND_CH && s2 < n;
  const double v = rhs[ok ? (FWD ? s2 : n - 1 - s2) : 0];
  c.nx = ok ? v : 0.0;
}

// PH = (s0 / 32) % 2 (the owner of step s0+i is lane (PH*32 + i) % M).
template <int M, int PH, int I>
__device__ __forceinline__ void band_step(const BandChunk& c, double& acc, double& done) {
  constexpr int owner = (PH * BAND_CH + I) & (M - 1);
  const double vk = readlane_f64(acc, owner);
  acc -= c.lc[I] * vk;  // lc == 0 outside the band and for the owner itself
  writelane_f64<I>(done, vk);
  writelane_f64<owner>(acc, readlane_f64(c.nx, I));
}
template <int M, int PH, int... I>
__device__ __forceinline__ void band_step_seq(const BandChunk& c, double& acc, double& done,
                                              std::integer_sequence<int, I...>) {
  (band_step<M, PH, I>(c, acc, done), ...);
}
template <int M, bool FWD, int PH>
__device__ __forceinline__ void band_steps(const BandChunk& c, double& acc, int64_t s0,
                                           int64_t n, int lane, double* __restrict__ x) {
  double done = 0.0;  // lane i collects the value finished at step s0+i
  band_step_seq<M, PH>(c, acc, done, std::make_integer_sequence<int, BAND_CH>{});
  const int64_t s = s0 + lane;
  if (lane < BAND_CH && s < n) x[FWD ? s : n - 1 - s] = done;
}

template <int M, bool FWD>
__device__ __forceinline__ void band_pass(int64_t n, int lane, const double* __restrict__ sched,
                                          const double* __restrict__ rhs, double* __restrict__ x) {
  double acc = 0.0;
  if (lane < M && lane < n) acc = FWD ? rhs[lane] : rhs[n - 1 - lane];
  BandChunk A, B;
  band_load<M, FWD>(A, 0, n, lane, sched, rhs);
  for (int64_t s0 = 0; s0 < n; s0 += 2 * BAND_CH) {  // s0 % 64 == 0
    band_load<M, FWD>(B, s0 + BAND_CH, n, lane, sched, rhs);
    band_steps<M, FWD, 0>(A, acc, s0, n, lane, x);
    band_load<M, FWD>(A, s0 + 2 * BAND_CH, n, lane, sched, rhs);
    band_steps<M, FWD, 1>(B, acc, s0 + BAND_CH, n, lane, x);
  }
}

// y: scratch vector of n doubles (forward result, then z = y / D).
template <int M>
__global__ __launch_bounds__(64) void band_solve_kernel(
    int64_t n, const double* __restrict__ sched_f, const double* __restrict__ sched_b,
    const double* __restrict__ dg, const double* __restrict__ f, double* __restrict__ y,
    double* __restrict__ x, int64_t cstride) {
  const int lane = threadIdx.x;
  const int64_t co = (int64_t)blockIdx.x * cstride;  // one workgroup per right-hand side (block cycle)
  f += co;
  y += co;
  x += co;
  band_pass<M, true>(n, lane, sched_f, f, y);           // L y = f
  __threadfence_block();
  for (int64_t i = lane; i < n; i += 64) y[i] = y[i] / dg[i];  // z = y / D
  __threadfence_block();
  band_pass<M, false>(n, lane, sched_b, y, x);          // L^T x = z
}

// ------------------------------------------------------------- K-BandChain ----
// The same substitution for the NARROW coarsest operators of deep hierarchies (half-bandwidth
// w <= 3, a few hundred rows: 511 rows / w = 2 on the 16-level 4096^2 hierarchy), where the
// broadcast-and-update scheme above spends ~48 ns per step on lane traffic.  Here the whole
// problem sits in LDS and every lane walks the recurrence redundantly as plain scalar code:
//   y_s = rhs_s - sum_t c[s][t] * y_{s-w+t},  t = 0 .. w-1  (ascending k, farthest first:
// the order in which K-Band's updates reach a row, so the bits are the same),
// with the operands of the next 8 steps read ahead of the dependent multiply / subtract chain
// (one multiply and one subtract per step on the critical path).  The backward pass runs the
// same code on the mirrored system (step s = row n-1-s; host_setup.cpp: band_chain_schedule).
constexpr int CHAIN_CH = 8;  // steps per read-ahead chunk
__host__ __device__ inline int band_chain_pad(int n) { return (n + 2 * CHAIN_CH - 1) / (2 * CHAIN_CH) * (2 * CHAIN_CH) + 2 * CHAIN_CH; }
template <int W>
struct ChainChunk {
  double o[CHAIN_CH][W], r[CHAIN_CH];
};
// ops / v are padded to band_chain_pad(n) steps (zero operands): no bounds checks on reads
template <int W>
__device__ __forceinline__ void band_chain_fetch(ChainChunk<W>& c, const double* op, const double* rv) {
#pragma unroll
  for (int i = 0; i < CHAIN_CH; ++i) {
#pragma unroll
    for (int t = 0; t < W; ++t) c.o[i][t] = op[i * W + t];
    c.r[i] = rv[i];
  }
}
// One chunk of CHAIN_CH steps of y_i = ((r_i - o[i][0] y_{i-W}) - ...) - o[i][W-1] y_{i-1} (ascending
// distance order: the row-oriented substitution's).  Only the LAST product depends on the previous
// step: a step's critical path is one multiply and one subtract (two dependent fp64 operations,
// ~11 cycles each on gfx950: tools/fp64_chain.hip).  Everything before that product -- the
// "early" part r_i - sum_{t < W-1} o[i][t] y_{i-W+t} -- only needs results that are at least two
// steps old, so the early part of step i+1 is formed while step i's chain is in flight, in a
// PINNED instruction order (an in-order wave executes what it is given; left to the scheduler
// the four operations of a step came out as one dependent sequence, 31 ns per step):
//   m = o[i][W-1] * y_{i-1};  products of early_{i+1};  y_i = early_i - m;  subtractions of early_{i+1}
// Same operations on the same operands in the same order per row: same bits.
// nxt: the chunk after c (its first step's early part is formed by c's last step).
template <int W>
__device__ __forceinline__ void band_chain_steps(const ChainChunk<W>& c, const ChainChunk<W>& nxt,
                                                 double (&prev)[W], double& early, int lane, double* out) {
  double res[CHAIN_CH];
#pragma unroll
  for (int i = 0; i < CHAIN_CH; ++i) {
    const double m = c.o[i][W - 1] * prev[W - 1];
    __builtin_amdgcn_sched_barrier(0);
    const double* on = i + 1 < CHAIN_CH ? c.o[i + 1] : nxt.o[0];
    double pr[W > 1 ? W - 1 : 1];
#pragma unroll
    for (int t = 0; t + 1 < W; ++t) pr[t] = on[t] * prev[t + 1];   // y_{i+1-W+t} = prev[t + 1]
    __builtin_amdgcn_sched_barrier(0);
    const double acc = early - m;
    __builtin_amdgcn_sched_barrier(0);
    double en = i + 1 < CHAIN_CH ? c.r[i + 1] : nxt.r[0];
#pragma unroll
    for (int t = 0; t + 1 < W; ++t) en -= pr[t];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int t = 0; t + 1 < W; ++t) prev[t] = prev[t + 1];
    prev[W - 1] = acc;
    res[i] = acc;
    early = en;
  }
  if (lane == 0) {  // every lane holds all eight results; one lane stores them (padded array)
#pragma unroll
    for (int i = 0; i < CHAIN_CH; ++i) out[i] = res[i];
  }
}
template <int W>
__device__ __forceinline__ void band_chain_pass(int n, const double* ops, double* v) {
  const int lane = threadIdx.x;
  double prev[W];
#pragma unroll
  for (int t = 0; t < W; ++t) prev[t] = 0.0;
  ChainChunk<W> A, B;
  band_chain_fetch<W>(A, ops, v);
  double early = A.r[0];  // step 0: the same subtractions of (operand x 0.0) the plain loop makes
#pragma unroll
  for (int t = 0; t + 1 < W; ++t) early -= A.o[0][t] * prev[t];
  for (int s0 = 0; s0 < n; s0 += 2 * CHAIN_CH) {
    const double* op = ops + s0 * W;
    double* rv = v + s0;
    // the next chunk's operands are read BEFORE this chunk's dependent chain starts (and stay
    // there: sched_barrier), so the LDS latency hides behind it
    band_chain_fetch<W>(B, op + CHAIN_CH * W, rv + CHAIN_CH);
    __builtin_amdgcn_sched_barrier(0);
    band_chain_steps<W>(A, B, prev, early, lane, rv);
    __builtin_amdgcn_sched_barrier(0);
    band_chain_fetch<W>(A, op + 2 * CHAIN_CH * W, rv + 2 * CHAIN_CH);
    __builtin_amdgcn_sched_barrier(0);
    band_chain_steps<W>(B, A, prev, early, lane, rv + CHAIN_CH);
    __builtin_amdgcn_sched_barrier(0);
  }
}
// The stand-alone launch: a workgroup of CHAIN_T threads (four waves, one per SIMD) around the
// recurrence, which wave 0 walks alone (tail_kernel's coarsest-solve block has the same form).
// Everything that is parallel -- staging, the scaling by D^-1, the store of x, the prolongation --
// is spread over all threads, and every global load the launch needs is issued at entry, before the
// first wait: ONE memory round trip ahead of the forward pass for up to 512 rows (the headline's
// 511), and none between the forward pass and the final stores.  Longer systems take further
// rounds, written as loops of a few loads issued together.
constexpr int CHAIN_T = 256;
// one round of a global -> LDS copy: R loads per thread issued together (entries base + j * CHAIN_T
// + tid below `valid`; past the end the last entry is read again and not stored: straight-line
// loads, no branch around each), and their LDS stores
template <int R>
__device__ __forceinline__ void band_chain_load(double (&t)[R], const double* __restrict__ src, int valid,
                                                int base, int tid) {
#pragma unroll
  for (int j = 0; j < R; ++j) {
    const int k = base + j * CHAIN_T + tid;
    t[j] = src[min(k, valid - 1)];
  }
}
template <int R>
__device__ __forceinline__ void band_chain_store(const double (&t)[R], double* dst, int valid, int base,
                                                 int tid) {
#pragma unroll
  for (int j = 0; j < R; ++j) {
    const int k = base + j * CHAIN_T + tid;
    if (k < valid) dst[k] = t[j];
  }
}
// the rounds after the first (whose loads the kernel issues at entry with everything else), and
// the zero operands of the padding
template <int R>
__device__ __forceinline__ void band_chain_stage_rest(const double* __restrict__ src, double* dst, int valid,
                                                      int total, int tid) {
  for (int base = CHAIN_T * R; base < valid; base += CHAIN_T * R) {
    double t[R];
    band_chain_load<R>(t, src, valid, base, tid);
    band_chain_store<R>(t, dst, valid, base, tid);
  }
  for (int k = valid + tid; k < total; k += CHAIN_T) dst[k] = 0.0;
}
template <int W>
__global__ __launch_bounds__(CHAIN_T) void band_chain_kernel(
    int n, const double* __restrict__ cf, const double* __restrict__ cb,
    const double* __restrict__ dg, const double* __restrict__ f, double* __restrict__ x, int n_h,
    const double* uh_in, double* uh_out, int pre, int64_t cstride) {
  extern __shared__ double chain_lds[];
  f += (int64_t)blockIdx.x * cstride;  // one workgroup per right-hand side (block cycle)
  x += (int64_t)blockIdx.x * cstride;
  const int np = band_chain_pad(n);
  double* ops = chain_lds;           // np x W: forward operands
  double* v = chain_lds + np * W;    // np: right-hand side in step order, then the result
  // backward operands: staged with the forward ones when the LDS allows (pre: no global round
  // trip between the two passes), else over them after the first pass
  double* opb = pre ? v + np : ops;
  const int tid = threadIdx.x;
  constexpr int RO = 4, RF = 2;      // loads per thread and round: operands (1024 entries), f (512)
  // ---- entry: every load of the launch's first round, then the first wait ----
  // the diagonal of the rows this thread scales between the passes: row tid and its mirror
  const int nhalf = (n + 1) / 2;
  double d_lo = dg[min(tid, n - 1)], d_hi = dg[max(n - 1 - tid, 0)];
  // the fine vector the result is prolonged into: two pairs per thread and round (1024 fine rows)
  double a0[2] = {0.0, 0.0}, a1[2] = {0.0, 0.0};
  auto fetch_fine = [&](int j0) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int i = 2 * (j0 + q * CHAIN_T + tid);  // past the end: the last row again, never stored
      a0[q] = uh_in[min(i, n_h - 1)];
      a1[q] = uh_in[min(i + 1, n_h - 1)];
    }
  };
  double tb[RO], tf[RF], to[RO];
  band_chain_load<RO>(tb, cb, n * W, 0, tid);   // stored now (pre) or after the forward pass
  band_chain_load<RF>(tf, f, n, 0, tid);
  band_chain_load<RO>(to, cf, n * W, 0, tid);
  if (uh_out) fetch_fine(0);
  band_chain_store<RO>(to, ops, n * W, 0, tid);
  band_chain_store<RF>(tf, v, n, 0, tid);
  band_chain_stage_rest<RO>(cf, ops, n * W, np * W, tid);
  band_chain_stage_rest<RF>(f, v, n, np, tid);
  if (pre) {
    band_chain_store<RO>(tb, opb, n * W, 0, tid);
    band_chain_stage_rest<RO>(cb, opb, n * W, np * W, tid);
  }
  lds_barrier();
  if (tid < 64) band_chain_pass<W>(n, ops, v);   // L y = f
  lds_barrier();
  // ---- z = y / D, mirrored: step s of the backward pass is row n-1-s.  A thread takes a row and
  // its mirror and swaps the two quotients in place: no other thread touches either entry ----
  for (int i = tid; i < nhalf; i += CHAIN_T) {
    const int m = n - 1 - i;
    if (i >= CHAIN_T) {  // rows past the entry round: n > 512
      d_lo = dg[i];
      d_hi = dg[m];
    }
    const double z_lo = v[i] / d_lo, z_hi = v[m] / d_hi;
    v[m] = z_lo;
    v[i] = z_hi;
  }
  if (!pre) {  // ops is free: cb goes over it, the first round from the registers loaded at entry
    band_chain_store<RO>(tb, opb, n * W, 0, tid);
    band_chain_stage_rest<RO>(cb, opb, n * W, n * W, tid);  // the padding still holds cf's zeros
  }
  lds_barrier();
  if (tid < 64) band_chain_pass<W>(n, opb, v);   // L^T x = z, step s = row n-1-s
  lds_barrier();
  // ---- exit: the sums of the first 1024 fine rows, then every store (stores count in vmcnt too:
  // a wait for a fine pair issued behind a store would wait for that store) ----
  // the prolongation into the level above (multigrid.hpp:294-296 for l = L-2), which would
  // otherwise be a launch of its own: uh_out = uh_in + P x, linear_prolong_add2_kernel's
  // expressions and order; x sits in v[] mirrored (x_j = v[n-1-j])
  double o0[2], o1[2];
  auto prolong_sums = [&](int j0) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int j = j0 + q * CHAIN_T + tid;
      double t0 = 0.0, t1 = 0.0;
      const double b = (j < n) ? v[n - 1 - j] : 0.0;
      if (j >= 1 && j - 1 < n) t0 += 0.5 * v[n - j];
      if (j < n) {
        t0 += 0.5 * b;
        t1 += 1.0 * b;
      }
      o0[q] = a0[q] + t0;
      o1[q] = a1[q] + t1;
    }
  };
  auto prolong_store = [&](int j0) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int i = 2 * (j0 + q * CHAIN_T + tid);
      if (i < n_h) uh_out[i] = o0[q];
      if (i + 1 < n_h) uh_out[i + 1] = o1[q];
    }
  };
  prolong_sums(0);  // without uh_out: sums onto zeros that nobody stores, and no branch
  for (int s = tid; s < n; s += CHAIN_T) x[n - 1 - s] = v[s];
  if (uh_out) {
    prolong_store(0);
    for (int j0 = CHAIN_T * 2; 2 * j0 < n_h; j0 += CHAIN_T * 2) {
      fetch_fine(j0);
      prolong_sums(j0);
      prolong_store(j0);
    }
  }
}
bool band_chain_ok(int64_t n, int64_t w) { return w >= 1 && w <= 3 && n >= 1 && n <= 2048; }
hipError_t launch_band_chain(int64_t n, int w, const double* cf, const double* cb, const double* dg,
                             const double* f, double* x, hipStream_t st, int64_t n_h, const double* uh_in,
                             double* uh_out, int cols, int64_t cstride) {
  if (!band_chain_ok(n, w) || (uh_out && (!uh_in || n_h < 1 || n_h > 2 * n + 2))) return hipErrorInvalidValue;
  if (cols < 1 || (uh_out && cols != 1)) return hipErrorInvalidValue;
  const size_t np = (size_t)band_chain_pad((int)n);
  const int pre = sizeof(double) * np * (size_t)(2 * w + 1) <= (size_t)48 * 1024 ? 1 : 0;
  const size_t lds = sizeof(double) * np * (size_t)(pre ? 2 * w + 1 : w + 1);
  switch (w) {
    case 1: hipLaunchKernelGGL(band_chain_kernel<1>, dim3(cols), dim3(CHAIN_T), lds, st, (int)n, cf, cb, dg, f, x, (int)n_h, uh_in, uh_out, pre, cstride); break;
    case 2: hipLaunchKernelGGL(band_chain_kernel<2>, dim3(cols), dim3(CHAIN_T), lds, st, (int)n, cf, cb, dg, f, x, (int)n_h, uh_in, uh_out, pre, cstride); break;
    default: hipLaunchKernelGGL(band_chain_kernel<3>, dim3(cols), dim3(CHAIN_T), lds, st, (int)n, cf, cb, dg, f, x, (int)n_h, uh_in, uh_out, pre, cstride); break;
  }
  return hipGetLastError();
}

// ------------------------------------------------------------------ K-Tail -----
// The deepest levels of a 2+2 true-Jacobi cycle in ONE launch of ONE workgroup (1024 threads),
// with every vector of those levels RESIDENT IN LDS: the down-legs of the levels lt .. L-2 (second
// pre-sweep, residual, restriction, first sweep of the next level), the coarsest solve
// (K-BandChain's recurrence on wave 0), the prolongation out of the coarsest level, the up-legs back
// to level lt and the prolongation into level lt - 1.  Every one of those steps is a launch of
// 5-7 us otherwise -- and almost all of that is latency: the launch itself and two or three
// dependent global round trips per step for a few thousand rows.  (A first form of this kernel
// that kept the vectors in global memory and replayed the pair kernels tile by tile inside one
// workgroup took 134 us for what eleven launches do in 70: the round trips, not the launches,
// are the cost.)  Here a step is an LDS pass and a workgroup barrier: row types, tables, f and
// the first-sweep result of level lt are staged once, everything else is produced in LDS; the
// level vectors leave for global memory once, at the end (the getters and the finer level read
// them there).  Same row arithmetic (dict_fetch / dict_rows on the same operands in the same
// order), same transfer expressions, same recurrence: same bits.  All levels run with the widest
// instantiation (two code words, nine slots); absent slots are no entries.
constexpr int TAIL_MAX_LEVELS = TAIL_LEVELS_MAX;
constexpr int TAIL_MAX_COARSE = 1024;
constexpr int TAIL_LDS_DOUBLES = 18432;   // 147 456 B
typedef TailLevelRef TailLevel;
typedef TailRef TailArgs;
int tail_max_coarse() { return TAIL_MAX_COARSE; }
__host__ __device__ inline int tail_pad(int n) { return (n + 3) & ~1; }   // even, one spare entry
// LDS layout in doubles: per level {U, F, tabJ (1024), tabR (1024), wtab (512), row types (n bytes)},
// then T and R (scratch of the largest level), Uc, the chain arrays
__host__ __device__ inline size_t tail_lds_doubles(const TailArgs& A) {
  size_t d = 0;
  int nmax = 0;
  for (int q = 0; q < A.nlev; ++q) {
    d += 2 * (size_t)tail_pad(A.L[q].n) + 1024 + 1024 + 512 + (size_t)((A.L[q].n + 15) / 16) * 2;
    nmax = A.L[q].n > nmax ? A.L[q].n : nmax;
  }
  d += 2 * (size_t)tail_pad(nmax) + (size_t)tail_pad(A.nc) + (size_t)band_chain_pad(A.nc) * (size_t)(A.wc + 1);
  return d;
}
// offsets (in doubles) into the kernel's one LDS array: pointers are formed from the array at
// every use, so the compiler knows the address space (ds_ instructions, not flat ones)
struct TailLds {
  int U, F, tabJ, tabR, wtab, rt;
};
// out[row] = the MODE operation on rows [0, n) of the level, x / f / out in LDS
template <int MODE>
__device__ __forceinline__ void tail_rows(int n, const DictEntry* tab, const uint64_t* wtab, const uint8_t* rt,
                                          const double* x, const double* f, double* out, double omega) {
  for (int row0 = (int)threadIdx.x * 2; row0 < n; row0 += 2048) {
    DictStream<2, 2> s;
    dict_fetch<MODE, 2, false, 2>(s, row0, n, nullptr, rt, f, x, 0);
    dict_expand<2, 2>(s, wtab);
    double res[2];
    dict_rows<MODE, 2, 9, 2>(s, row0, tab, x, omega, 0, res);
    if (s.live[0]) out[row0] = res[0];
    if (s.live[1]) out[row0 + 1] = res[1];
  }
}
// out[i] = base[i] + (P uH)[i] for i in [0, n_h) (linear_prolong_add2_kernel)
__device__ __forceinline__ void tail_prolong(int n_h, int n_H, const double* uH, const double* base, double* out) {
  for (int j = threadIdx.x; 2 * j < n_h; j += 1024) {
    const int i = 2 * j;
    double t0 = 0.0, t1 = 0.0;
    const double b = (j < n_H) ? uH[j] : 0.0;
    if (j >= 1 && j - 1 < n_H) t0 += 0.5 * uH[j - 1];
    if (j < n_H) {
      t0 += 0.5 * b;
      t1 += 1.0 * b;
    }
    out[i] = base[i] + t0;
    if (i + 1 < n_h) out[i + 1] = base[i + 1] + t1;
  }
}
template <int W>
__global__ __launch_bounds__(1024) void tail_kernel(TailArgs A) {
  __shared__ __attribute__((aligned(16))) double tail_lds[TAIL_LDS_DOUBLES];   // static: 144 KB of the CU's 160
  TailLds P[TAIL_MAX_LEVELS];
  int p = 0, nmax = 0;
  for (int q = 0; q < A.nlev; ++q) {
    const int n = A.L[q].n, np = tail_pad(n);
    P[q].U = p; p += np;
    P[q].F = p; p += np;
    P[q].tabJ = p; p += 1024;
    P[q].tabR = p; p += 1024;
    P[q].wtab = p; p += 512;
    P[q].rt = p; p += ((n + 15) / 16) * 2;
    nmax = n > nmax ? n : nmax;
  }
  double* const T = tail_lds + p; p += tail_pad(nmax);
  double* const R = tail_lds + p; p += tail_pad(nmax);
  const int Uc = p; p += tail_pad(A.nc);
  const int npc = band_chain_pad(A.nc);
  double* const ops = tail_lds + p;      // npc x W
  const int voff = p + npc * W;
  double* const v = tail_lds + voff;     // npc: coarsest right-hand side in step order, then the result
  if (voff + npc > TAIL_LDS_DOUBLES) return;   // launch_tail refuses such a hierarchy; never reached
  const double omega = A.omega;
  const int tid = (int)threadIdx.x;
#define TAIL_D(off) (tail_lds + (off))
#define TAIL_TAB(off) reinterpret_cast<DictEntry*>(tail_lds + (off))
#define TAIL_W(off) reinterpret_cast<uint64_t*>(tail_lds + (off))
#define TAIL_B(off) reinterpret_cast<uint8_t*>(tail_lds + (off))
  // ---- stage: tables and row types of every level, f and the first-sweep result of level lt, the
  // forward operands of the coarsest factor -- all requested before the first wait ----
  for (int q = 0; q < A.nlev; ++q) {
    const TailLevel& L = A.L[q];
    if (tid < 256) {
      const int t = tid;
      const double val = t < L.ntab ? L.dval[t] : 0.0;
      const int32_t o = t < L.ntab ? L.doff[t] : 0;
      DictEntry e;
      e.a = o == 0 ? 0.0 : val;                    // dict_stage_table<CSR_JACOBI>
      e.d = (o == 0 && t < L.ntab) ? val : 0.0;
      e.off8 = o * 8;
      e.pad[0] = e.pad[1] = e.pad[2] = 0;
      TAIL_TAB(P[q].tabJ)[t] = e;
      e.a = val;                                   // dict_stage_table<CSR_RESID>
      e.d = 0.0;
      TAIL_TAB(P[q].tabR)[t] = e;
      TAIL_W(P[q].wtab)[2 * t] = L.rwords[(size_t)t * L.words];
      TAIL_W(P[q].wtab)[2 * t + 1] = L.words == 2 ? L.rwords[(size_t)t * 2 + 1] : ~(uint64_t)0;
    }
    for (int r = tid; r < ((L.n + 15) / 16) * 16; r += 1024) TAIL_B(P[q].rt)[r] = r < L.n ? L.rtype[r] : (uint8_t)255;
  }
  for (int r = tid; r < tail_pad(A.L[0].n); r += 1024) {
    TAIL_D(P[0].F)[r] = r < A.L[0].n ? A.L[0].f[r] : 0.0;
    T[r] = r < A.L[0].n ? A.L[0].tmp[r] : 0.0;
  }
  for (int k = tid; k < npc * W; k += 1024) ops[k] = k < A.nc * W ? A.cf[k] : 0.0;
  __syncthreads();
  // ---- down-legs (multigrid.hpp:265-283) ----
  for (int li = 0; li < A.nlev; ++li) {
    const int n = A.L[li].n;
    const bool last = li + 1 == A.nlev;
    const int nH = last ? A.nc : A.L[li + 1].n;
    const double* dH = last ? A.diagc : A.L[li + 1].diag;
    const TailLds Q = P[li];
    tail_rows<CSR_JACOBI>(n, TAIL_TAB(Q.tabJ), TAIL_W(Q.wtab), TAIL_B(Q.rt), T, TAIL_D(Q.F), TAIL_D(Q.U),
                          omega);                                          // second pre-sweep (T = the first)
    __syncthreads();
    tail_rows<CSR_RESID>(n, TAIL_TAB(Q.tabR), TAIL_W(Q.wtab), TAIL_B(Q.rt), TAIL_D(Q.U), TAIL_D(Q.F), R,
                         omega);                                           // r = f - A u
    if (tid < 2) R[n + tid] = 0.0;
    __syncthreads();
    double* FH = TAIL_D(last ? voff : P[li + 1 < A.nlev ? li + 1 : li].F);
    for (int j = tid; j < nH; j += 1024) {                                // linear_restrict_kernel + jacobi_from_zero
      const int i = 2 * j;
      double sum = 0.0;
      if (i < n) sum += 0.5 * R[i];
      if (i + 1 < n) sum += 1.0 * R[i + 1];
      if (i + 2 < n) sum += 0.5 * R[i + 2];
      FH[j] = sum;
      const double xi = 0.0, acc = 0.0;
      const double d = dH[j];
      T[j] = (d == 0.0) ? xi : xi + omega * ((sum - acc) / d - xi);
    }
    if (last)
      for (int j = nH + tid; j < npc; j += 1024) v[j] = 0.0;
    __syncthreads();
  }
  // ---- coarsest solve (multigrid.hpp:287-288): band_chain_kernel, wave 0 walks the recurrence ----
  {
    const int n = A.nc;
    if (tid >= 64)   // the level's right-hand side and first sweep go home while wave 0 solves
      for (int j = tid - 64; j < n; j += 960) {
        A.fc[j] = v[j];
        A.tmpc[j] = T[j];
      }
    __syncthreads();
    if (tid < 64) band_chain_pass<W>(n, ops, v);       // L y = f
    __syncthreads();
    double z = 0.0;
    if (tid < n) z = v[n - 1 - tid] / A.dg[n - 1 - tid];
    for (int k = tid; k < n * W; k += 1024) ops[k] = A.cb[k];
    __syncthreads();
    if (tid < n) v[tid] = z;
    __syncthreads();
    if (tid < 64) band_chain_pass<W>(n, ops, v);       // L^T x = z, step s = row n-1-s
    __syncthreads();
    if (tid < n) {
      const double x = v[tid];
      TAIL_D(Uc)[n - 1 - tid] = x;
      A.uc[n - 1 - tid] = x;
    }
    __syncthreads();
  }
  // ---- up-legs (multigrid.hpp:291-302) ----
  int uH = Uc;
  int nH = A.nc;
  for (int li = A.nlev - 1; li >= 0; --li) {
    const int n = A.L[li].n;
    const TailLds Q = P[li];
    tail_prolong(n, nH, TAIL_D(uH), TAIL_D(Q.U), T);                       // T = u + P u_H
    __syncthreads();
    tail_rows<CSR_JACOBI>(n, TAIL_TAB(Q.tabJ), TAIL_W(Q.wtab), TAIL_B(Q.rt), T, TAIL_D(Q.F), R, omega);
    __syncthreads();
    tail_rows<CSR_JACOBI>(n, TAIL_TAB(Q.tabJ), TAIL_W(Q.wtab), TAIL_B(Q.rt), R, TAIL_D(Q.F), TAIL_D(Q.U), omega);
    __syncthreads();
    uH = Q.U;
    nH = n;
  }
  // ---- the prolongation into level lt - 1, and the level vectors go home ----
  tail_prolong(A.n_fine, nH, TAIL_D(uH), A.uf_in, A.uf_out);
  for (int li = 0; li < A.nlev; ++li) {
    const TailLevel& L = A.L[li];
    for (int r = tid; r < L.n; r += 1024) {
      L.u[r] = TAIL_D(P[li].U)[r];
      if (li > 0) const_cast<double*>(L.f)[r] = TAIL_D(P[li].F)[r];
    }
  }
#undef TAIL_D
#undef TAIL_TAB
#undef TAIL_W
#undef TAIL_B
}
bool tail_level_ok(int64_t n, const DictRef& D, int hb) {
  return D.rtype && D.rwords && !D.nt && hb >= 0 && n >= 256 && n <= 4095 && D.wmax <= 9 && D.words >= 1 &&
         D.words <= 2 && D.ntab <= 255;
}
size_t tail_lds_bytes(const TailRef& A) { return sizeof(double) * tail_lds_doubles(A); }
size_t tail_lds_capacity() { return sizeof(double) * (size_t)TAIL_LDS_DOUBLES; }
hipError_t launch_tail(const TailArgs& A, hipStream_t st) {
  if (A.nlev < 1 || A.nlev > TAIL_MAX_LEVELS || A.nc < 1 || A.nc > TAIL_MAX_COARSE || !band_chain_ok(A.nc, A.wc) ||
      tail_lds_bytes(A) > tail_lds_capacity() || A.n_fine < 1 || !A.uf_in || !A.uf_out)
    return hipErrorInvalidValue;
  for (int q = 0; q < A.nlev; ++q)
    if (A.L[q].n < 2 || !A.L[q].rtype || !A.L[q].rwords || !A.L[q].doff || !A.L[q].dval || !A.L[q].f || !A.L[q].u ||
        !A.L[q].tmp || !A.L[q].diag || A.L[q].ntab < 1 || A.L[q].ntab > 255)
      return hipErrorInvalidValue;
  switch (A.wc) {
    case 1: hipLaunchKernelGGL(tail_kernel<1>, dim3(1), dim3(1024), 0, st, A); break;
    case 2: hipLaunchKernelGGL(tail_kernel<2>, dim3(1), dim3(1024), 0, st, A); break;
    default: hipLaunchKernelGGL(tail_kernel<3>, dim3(1), dim3(1024), 0, st, A); break;
  }
  return hipGetLastError();
}

// ------------------------------------------------------------- K-BandWide -----
// The same LDL^T substitution for ANY half-bandwidth w (the reference's SimplicialLDLT
// factors whatever coarsest matrix it is given, multigrid.hpp:240-243): rows in blocks of
// 64, one wave, lane l owns row r0 + l of the current block.
//   phase 1: the terms that come from earlier blocks, k = i-w .. r0-1 in ascending k --
//            a private loop per lane over the block's [t][lane] operand panel (coalesced
//            512-B loads), y_k from an LDS ring that holds the last w + 64 results;
//   phase 2: the 64 x 64 triangle of the block itself, step s broadcasts the finished
//            y_{r0+s} with v_readlane (ascending k again).
// Every row therefore subtracts its products in exactly the order of the row-oriented
// substitution (oracle band_solve), so the result has the same bits.  The backward pass
// runs the same code on the mirrored system (row n-1-i, host_setup.cpp: band_wide_schedule).
template <bool FWD>
__device__ __forceinline__ void band_wide_pass(int64_t n, int w, int ringmask, double* ring,
                                               const double* __restrict__ sched,
                                               const double* rhs, double* out) {
  const int lane = threadIdx.x;
  const int64_t nb = (n + 63) / 64;
  const int64_t stride = (int64_t)(w + 64) * 64;
  for (int k = lane; k <= ringmask; k += 64) ring[k] = 0.0;
  __syncthreads();
  for (int64_t b = 0; b < nb; ++b) {
    const int64_t r0 = b * 64, i = r0 + lane;
    const bool live = i < n;
    double acc = live ? rhs[FWD ? i : n - 1 - i] : 0.0;
    const double* __restrict__ Lp = sched + b * stride + lane;
    const int64_t tl = (int64_t)w - i;
    const int tlo = tl > 0 ? (int)tl : 0, thi = w - lane;  // k >= 0 and k < r0
    if (b > 0) {
#pragma unroll 4
      for (int t = 0; t < w; ++t) {
        const double v = Lp[(int64_t)t * 64];
        const double yk = ring[(int)((i - w + t) & ringmask)];
        const double p = v * yk;
        acc = (t >= tlo && t < thi) ? acc - p : acc;
      }
    }
    const double* __restrict__ Ld = Lp + (int64_t)w * 64;
#pragma unroll 16
    for (int s = 0; s < 64; ++s) {
      const double vk = readlane_f64(acc, s);
      const double p = Ld[s * 64] * vk;
      acc = (lane > s) ? acc - p : acc;
    }
    if (live) {
      ring[(int)(i & ringmask)] = acc;
      out[FWD ? i : n - 1 - i] = acc;
    }
    __syncthreads();
  }
}
__global__ __launch_bounds__(64) void band_wide_kernel(
    int64_t n, int w, int ringmask, const double* __restrict__ sched_f,
    const double* __restrict__ sched_b, const double* __restrict__ dg, const double* f, double* y,
    double* x, int64_t cstride) {
  extern __shared__ double ring[];
  const int64_t co = (int64_t)blockIdx.x * cstride;  // one workgroup per right-hand side (block cycle)
  f += co;
  y += co;
  x += co;
  band_wide_pass<true>(n, w, ringmask, ring, sched_f, f, y);   // L y = f
  __threadfence_block();
  for (int64_t i = threadIdx.x; i < n; i += 64) y[i] = y[i] / dg[i];  // z = y / D
  __threadfence_block();
  __syncthreads();
  band_wide_pass<false>(n, w, ringmask, ring, sched_b, y, x);  // L^T x = z
}
hipError_t launch_band_wide(int64_t n, int64_t w, const double* sched_f, const double* sched_b,
                            const double* dg, const double* f, double* y, double* x,
                            hipStream_t st, int cols, int64_t cstride) {
  if (n <= 0) return hipSuccess;
  if (cols < 1) return hipErrorInvalidValue;
  int64_t R = 128;
  while (R < w + 64) R *= 2;
  if (R * 8 > 65536 || w < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(band_wide_kernel, dim3(cols), dim3(64), (size_t)R * 8, st, n, (int)w, (int)(R - 1),
                     sched_f, sched_b, dg, f, y, x, cstride);
  return hipGetLastError();
}

// ---------------------------------------------------------------- K-Spike -----
// Parallel form of the same LDL^T solve (host_setup.cpp: spike_factor): P partitions
// of c rows.  (A) every partition runs the one-wave substitution above on its own
// triangular block, one workgroup per partition; (B) one wave walks the P partition
// boundaries (w unknowns each: t_p = tail(g_p) - Vt_p t_{p-1}); (C) every row
// subtracts its spike row times the neighbouring boundary vector and divides by D;
// (D)-(F) mirror it for L^T.  Depth ~ 2c + P steps instead of n.  Same direct solve,
// different rounding order, so the V-cycle uses it only on request.
template <int M, bool FWD>
__global__ __launch_bounds__(64) void spike_local_kernel(SpikeArgs a, const double* rhs,
                                                         double* out) {
  const int lane = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * a.c;
  const int64_t nl = (a.n - r0 < a.c) ? a.n - r0 : a.c;
  band_pass<M, FWD>(nl, lane, (FWD ? a.sched_f : a.sched_b) + (int64_t)blockIdx.x * a.sched_stride,
                    rhs + r0, out + r0);
}
// forward: q = 0..P-1, block = last w rows of partition q, couples to q-1
// backward: q = P-1..0, block = first w rows of partition q, couples to q+1
// Vt/Wh blocks are zero-padded to M x M ([j][k], k fastest), so the matvec is a
// fixed-length unrolled loop and the next block is fetched while this one is used.
template <int M, bool FWD>
__global__ __launch_bounds__(64) void spike_boundary_kernel(SpikeArgs a, const double* g,
                                                            double* bnd) {
  const int k = threadIdx.x;
  const int w = a.w, wq = a.w > 0 ? a.w : 1;
  const bool act = k < w;
  const int kc = k < M ? k : 0;
  const double* blocks = FWD ? a.Vt : a.Wh;
  double cur[M], nxt[M];
#pragma unroll
  for (int j = 0; j < M; ++j) cur[j] = 0.0;
  double t = 0.0;
  for (int s = 0; s < a.P; ++s) {
    const int q = FWD ? s : a.P - 1 - s;
    const int64_t r0 = (int64_t)q * a.c;
    const int64_t nl = (a.n - r0 < a.c) ? a.n - r0 : a.c;
    const int64_t row = FWD ? r0 + nl - w + k : r0 + k;
    const bool ok = act && row >= r0 && row < r0 + nl;
    double v = g[ok ? row : 0];
    v = ok ? v : 0.0;
    if (s + 1 < a.P) {
      const double* blk = blocks + (int64_t)(FWD ? q + 1 : q - 1) * M * M + kc;
#pragma unroll
      for (int j = 0; j < M; ++j) nxt[j] = blk[j * M];
    }
#pragma unroll
    for (int j = 0; j < M; ++j) v -= cur[j] * readlane_f64(t, j);
    v = ok ? v : 0.0;
    if (act) bnd[(int64_t)q * wq + k] = v;
    t = v;
#pragma unroll
    for (int j = 0; j < M; ++j) cur[j] = nxt[j];
  }
}
// forward: out_i = (g_i - V_i . T[p-1]) / D_i ; backward: out_i = g_i - W_i . H[p+1]
template <bool FWD>
__global__ __launch_bounds__(256) void spike_correct_kernel(SpikeArgs a, const double* g,
                                                            const double* bnd, double* out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  const int w = a.w, wq = a.w > 0 ? a.w : 1;
  const int64_t p = i / a.c;
  double v = g[i];
  const int64_t nb = FWD ? p - 1 : p + 1;
  if (nb >= 0 && nb < a.P) {
    const double* __restrict__ sp = (FWD ? a.V : a.W) + i * wq;
    const double* __restrict__ t = bnd + nb * wq;
#pragma unroll 8
    for (int j = 0; j < w; ++j) v -= sp[j] * t[j];
  }
  out[i] = FWD ? v / a.d[i] : v;
}
template <int M>
static hipError_t launch_spike_m(const SpikeArgs& a, hipStream_t st) {
  const unsigned P = (unsigned)a.P, g = (unsigned)((a.n + 255) / 256);
  hipLaunchKernelGGL((spike_local_kernel<M, true>), dim3(P), dim3(64), 0, st, a, a.f, a.G);
  hipLaunchKernelGGL((spike_boundary_kernel<M, true>), dim3(1), dim3(64), 0, st, a, a.G, a.T);
  hipLaunchKernelGGL((spike_correct_kernel<true>), dim3(g), dim3(256), 0, st, a, a.G, a.T, a.Z);
  hipLaunchKernelGGL((spike_local_kernel<M, false>), dim3(P), dim3(64), 0, st, a, a.Z, a.G);
  hipLaunchKernelGGL((spike_boundary_kernel<M, false>), dim3(1), dim3(64), 0, st, a, a.G, a.H);
  hipLaunchKernelGGL((spike_correct_kernel<false>), dim3(g), dim3(256), 0, st, a, a.G, a.H, a.x);
  return hipGetLastError();
}
hipError_t launch_spike_solve(const SpikeArgs& a, hipStream_t st) {
  if (a.n <= 0) return hipSuccess;
  switch (a.m) {
    case 4: return launch_spike_m<4>(a, st);
    case 8: return launch_spike_m<8>(a, st);
    case 16: return launch_spike_m<16>(a, st);
    case 32: return launch_spike_m<32>(a, st);
    case 64: return launch_spike_m<64>(a, st);
  }
  return hipErrorInvalidValue;
}

hipError_t launch_band_solve(int64_t n, int m, const double* sched_f, const double* sched_b,
                             const double* dg, const double* f, double* y, double* x,
                             hipStream_t st, int cols, int64_t cstride) {
  if (n <= 0) return hipSuccess;
  if (cols < 1) return hipErrorInvalidValue;
  switch (m) {
    case 4: hipLaunchKernelGGL(band_solve_kernel<4>, dim3(cols), dim3(64), 0, st, n, sched_f, sched_b, dg, f, y, x, cstride); break;
    case 8: hipLaunchKernelGGL(band_solve_kernel<8>, dim3(cols), dim3(64), 0, st, n, sched_f, sched_b, dg, f, y, x, cstride); break;
    case 16: hipLaunchKernelGGL(band_solve_kernel<16>, dim3(cols), dim3(64), 0, st, n, sched_f, sched_b, dg, f, y, x, cstride); break;
    case 32: hipLaunchKernelGGL(band_solve_kernel<32>, dim3(cols), dim3(64), 0, st, n, sched_f, sched_b, dg, f, y, x, cstride); break;
    case 64: hipLaunchKernelGGL(band_solve_kernel<64>, dim3(cols), dim3(64), 0, st, n, sched_f, sched_b, dg, f, y, x, cstride); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

// ------------------------------------------------------------ K-Galerkin -----
// Setup on the device: A_H = R (A P) for the LinearInterpolator pair (P column j =
// {0.5, 1, 0.5} on rows 2j..2j+2, R = P^T; multigrid.hpp:219-223), in Eigen's
// conservative-product order: an output entry exists as soon as one product touches
// it (exact zeros are kept), its first product is assigned and the others are added in
// ascending inner index -- the same bits as host_setup.cpp: spgemm_csr.  Thread per
// output row, two passes (count, fill) around an exclusive scan.
//
// Row i of A P.  Walking A's row in ascending k, the coarse columns that P's row k
// holds (k odd: (k-1)/2; k even: k/2 - 1 and k/2) come out in non-decreasing order, so
// one open accumulator is enough.
template <bool FILL>
__global__ __launch_bounds__(256) void galerkin_ap_kernel(
    int64_t n_h, int64_t n_H, const int32_t* __restrict__ arp, const int32_t* __restrict__ acol,
    const double* __restrict__ aval, int32_t* __restrict__ cnt, const int32_t* __restrict__ orp,
    int32_t* __restrict__ ocol, double* __restrict__ oval) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_h) return;
  int32_t n_out = 0;
  int64_t cur = -1;
  double acc = 0.0;
  const int64_t base = FILL ? orp[i] : 0;
  auto touch = [&](int64_t c, double t) {
    if (c == cur) {
      acc += t;
    } else {
      if (cur >= 0) {
        if (FILL) { ocol[base + n_out] = (int32_t)cur; oval[base + n_out] = acc; }
        ++n_out;
      }
      cur = c;
      acc = t;  // first touch: assign
    }
  };
  for (int32_t p = arp[i]; p < arp[i + 1]; ++p) {
    const int64_t k = acol[p];
    const double a = aval[p];
    if (k & 1) {
      const int64_t c = (k - 1) >> 1;
      if (c < n_H) touch(c, a * 1.0);
    } else {
      const int64_t c = k >> 1;
      if (c >= 1 && c - 1 < n_H) touch(c - 1, a * 0.5);  // P(2(c-1)+2, c-1)
      if (c < n_H) touch(c, a * 0.5);                    // P(2c, c)
    }
  }
  if (cur >= 0) {
    if (FILL) { ocol[base + n_out] = (int32_t)cur; oval[base + n_out] = acc; }
    ++n_out;
  }
  if (!FILL) cnt[i] = n_out;
}
// Row j of R (A P): three-way merge of rows 2j, 2j+1, 2j+2 of A P, products taken in
// that order (R's row j in ascending column).
template <bool FILL>
__global__ __launch_bounds__(256) void galerkin_rap_kernel(
    int64_t n_h, int64_t n_H, const int32_t* __restrict__ prp, const int32_t* __restrict__ pcol,
    const double* __restrict__ pval, int32_t* __restrict__ cnt, const int32_t* __restrict__ orp,
    int32_t* __restrict__ ocol, double* __restrict__ oval) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n_H) return;
  const double w[3] = {0.5, 1.0, 0.5};
  int32_t q[3], e[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const int64_t i = 2 * j + r;
    q[r] = i < n_h ? prp[i] : 0;
    e[r] = i < n_h ? prp[i + 1] : 0;
  }
  int32_t n_out = 0;
  const int64_t base = FILL ? orp[j] : 0;
  for (;;) {
    int32_t c = INT32_MAX;
#pragma unroll
    for (int r = 0; r < 3; ++r)
      if (q[r] < e[r]) { const int32_t cc = pcol[q[r]]; c = cc < c ? cc : c; }
    if (c == INT32_MAX) break;
    double v = 0.0;
    bool started = false;
#pragma unroll
    for (int r = 0; r < 3; ++r)
      if (q[r] < e[r] && pcol[q[r]] == c) {
        const double t = w[r] * pval[q[r]];
        v = started ? v + t : t;
        started = true;
        ++q[r];
      }
    if (FILL) { ocol[base + n_out] = c; oval[base + n_out] = v; }
    ++n_out;
  }
  if (!FILL) cnt[j] = n_out;
}
// General C = A B on CSR arrays (custom interpolators: A P and R (A P), multigrid.hpp:219-223)
// in Eigen's conservative-product order: row i of C is the K-way merge of the rows B[k, :] for
// the K entries k of A's row i; an output entry exists as soon as one product touches it, its
// first product is assigned and the later ones are added in ascending k (= the order of A's
// row) -- the same bits as host_setup.cpp: spgemm_csr.  Thread per output row, K <= 32 cursors
// (rows of A longer than that raise *overflow and the host product is used instead).
constexpr int SPGEMM_K = 32;
template <bool FILL>
__global__ __launch_bounds__(128) void spgemm_kway_kernel(
    int64_t n_rows, const int32_t* __restrict__ arp, const int32_t* __restrict__ acol,
    const double* __restrict__ aval, const int32_t* __restrict__ brp, const int32_t* __restrict__ bcol,
    const double* __restrict__ bval, int32_t* __restrict__ cnt, const int32_t* __restrict__ orp,
    int32_t* __restrict__ ocol, double* __restrict__ oval, int32_t* __restrict__ overflow) {
  const int64_t i = (int64_t)blockIdx.x * 128 + threadIdx.x;
  if (i >= n_rows) return;
  const int32_t a0 = arp[i], K = arp[i + 1] - a0;
  if (K > SPGEMM_K) {
    if (!FILL) cnt[i] = 0;
    atomicOr(overflow, 1);
    return;
  }
  int32_t q[SPGEMM_K], e[SPGEMM_K];
  for (int t = 0; t < K; ++t) {
    const int32_t k = acol[a0 + t];
    q[t] = brp[k];
    e[t] = brp[k + 1];
  }
  int32_t n_out = 0;
  const int64_t base = FILL ? orp[i] : 0;
  for (;;) {
    int32_t c = INT32_MAX;
    for (int t = 0; t < K; ++t)
      if (q[t] < e[t]) {
        const int32_t cc = bcol[q[t]];
        c = cc < c ? cc : c;
      }
    if (c == INT32_MAX) break;
    double v = 0.0;
    bool started = false;
    for (int t = 0; t < K; ++t)
      if (q[t] < e[t] && bcol[q[t]] == c) {
        if (FILL) {
          const double p = aval[a0 + t] * bval[q[t]];
          v = started ? v + p : p;
          started = true;
        }
        ++q[t];
      }
    if (FILL) {
      ocol[base + n_out] = c;
      oval[base + n_out] = v;
    }
    ++n_out;
  }
  if (!FILL) cnt[i] = n_out;
}
hipError_t launch_spgemm(bool fill, int64_t n_rows, const int32_t* arp, const int32_t* acol,
                         const double* aval, const int32_t* brp, const int32_t* bcol, const double* bval,
                         int32_t* cnt, const int32_t* orp, int32_t* ocol, double* oval,
                         int32_t* overflow, hipStream_t st) {
  const unsigned grid = (unsigned)((n_rows + 127) / 128);
  if (fill)
    hipLaunchKernelGGL(spgemm_kway_kernel<true>, dim3(grid), dim3(128), 0, st, n_rows, arp, acol, aval, brp,
                       bcol, bval, cnt, orp, ocol, oval, overflow);
  else
    hipLaunchKernelGGL(spgemm_kway_kernel<false>, dim3(grid), dim3(128), 0, st, n_rows, arp, acol, aval,
                       brp, bcol, bval, cnt, orp, ocol, oval, overflow);
  return hipGetLastError();
}
// exclusive scan of n int32 counts into n + 1 offsets (three small kernels)
__global__ __launch_bounds__(256) void scan_block_sums_kernel(int64_t n, const int32_t* __restrict__ in,
                                                              int64_t* __restrict__ bsum) {
  __shared__ int64_t red[256];
  const int64_t b0 = (int64_t)blockIdx.x * 1024;
  int64_t sum = 0;
  for (int k = 0; k < 4; ++k) {
    const int64_t i = b0 + threadIdx.x * 4 + k;
    if (i < n) sum += in[i];
  }
  red[threadIdx.x] = sum;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) bsum[blockIdx.x] = red[0];
}
// exclusive scan of the <= 2^21 block sums by ONE workgroup: thread t owns a contiguous
// run of ceil(nb / 1024) sums, the 1024 run totals are scanned in LDS
__global__ __launch_bounds__(1024) void scan_block_offsets_kernel(int64_t nb, int64_t* bsum,
                                                                  int64_t* total) {
  __shared__ int64_t part[1024];
  const int t = threadIdx.x;
  const int64_t per = (nb + 1023) / 1024;
  const int64_t b0 = (int64_t)t * per;
  const int64_t b1 = b0 + per < nb ? b0 + per : nb;
  int64_t s = 0;
  for (int64_t b = b0; b < b1; ++b) s += bsum[b];
  part[t] = s;
  __syncthreads();
  for (int st = 1; st < 1024; st <<= 1) {
    const int64_t add = t >= st ? part[t - st] : 0;
    __syncthreads();
    part[t] += add;
    __syncthreads();
  }
  int64_t run = part[t] - s;
  for (int64_t b = b0; b < b1; ++b) {
    const int64_t v = bsum[b];
    bsum[b] = run;
    run += v;
  }
  if (t == 1023) *total = part[1023];
}
__global__ __launch_bounds__(256) void scan_finish_kernel(int64_t n, const int32_t* __restrict__ in,
                                                          const int64_t* __restrict__ bsum,
                                                          int32_t* __restrict__ out) {
  __shared__ int64_t pre[256];
  const int64_t b0 = (int64_t)blockIdx.x * 1024;
  int32_t v[4];
  int64_t sum = 0;
  for (int k = 0; k < 4; ++k) {
    const int64_t i = b0 + threadIdx.x * 4 + k;
    v[k] = i < n ? in[i] : 0;
    sum += v[k];
  }
  pre[threadIdx.x] = sum;
  __syncthreads();
  for (int st = 1; st < 256; st <<= 1) {  // inclusive scan of the per-thread sums
    const int64_t add = (int)threadIdx.x >= st ? pre[threadIdx.x - st] : 0;
    __syncthreads();
    pre[threadIdx.x] += add;
    __syncthreads();
  }
  int64_t run = bsum[blockIdx.x] + pre[threadIdx.x] - sum;
  for (int k = 0; k < 4; ++k) {
    const int64_t i = b0 + threadIdx.x * 4 + k;
    if (i < n) out[i] = (int32_t)run;
    run += v[k];
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 255) out[n] = (int32_t)run;
}
// counts[0..n) -> offsets[0..n]; *total (device int64) = offsets[n]; bsum: ceil(n/1024) int64
hipError_t launch_exclusive_scan(int64_t n, const int32_t* counts, int32_t* offsets, int64_t* bsum,
                                 int64_t* total, hipStream_t st) {
  if (n <= 0) return hipErrorInvalidValue;
  const int64_t nb = (n + 1023) / 1024;
  hipLaunchKernelGGL(scan_block_sums_kernel, dim3((unsigned)nb), dim3(256), 0, st, n, counts, bsum);
  hipLaunchKernelGGL(scan_block_offsets_kernel, dim3(1), dim3(1024), 0, st, nb, bsum, total);
  hipLaunchKernelGGL(scan_finish_kernel, dim3((unsigned)nb), dim3(256), 0, st, n, counts, bsum,
                     offsets);
  return hipGetLastError();
}
hipError_t launch_galerkin_ap(bool fill, int64_t n_h, int64_t n_H, const int32_t* arp,
                              const int32_t* acol, const double* aval, int32_t* cnt,
                              const int32_t* orp, int32_t* ocol, double* oval, hipStream_t st) {
  const unsigned grid = (unsigned)((n_h + 255) / 256);
  if (fill)
    hipLaunchKernelGGL(galerkin_ap_kernel<true>, dim3(grid), dim3(256), 0, st, n_h, n_H, arp, acol,
                       aval, cnt, orp, ocol, oval);
  else
    hipLaunchKernelGGL(galerkin_ap_kernel<false>, dim3(grid), dim3(256), 0, st, n_h, n_H, arp, acol,
                       aval, cnt, orp, ocol, oval);
  return hipGetLastError();
}
hipError_t launch_galerkin_rap(bool fill, int64_t n_h, int64_t n_H, const int32_t* prp,
                               const int32_t* pcol, const double* pval, int32_t* cnt,
                               const int32_t* orp, int32_t* ocol, double* oval, hipStream_t st) {
  const unsigned grid = (unsigned)((n_H + 255) / 256);
  if (fill)
    hipLaunchKernelGGL(galerkin_rap_kernel<true>, dim3(grid), dim3(256), 0, st, n_h, n_H, prp, pcol,
                       pval, cnt, orp, ocol, oval);
  else
    hipLaunchKernelGGL(galerkin_rap_kernel<false>, dim3(grid), dim3(256), 0, st, n_h, n_H, prp, pcol,
                       pval, cnt, orp, ocol, oval);
  return hipGetLastError();
}

// ------------------------------------------------------- K-TensorGalerkin -----
// A_H = R (A P) for the full-coarsening pair (host_setup.hpp: tensor_P; R = P^T) from a general
// CSR(A) on the fine grid.  P, R and A P are never stored: P(k, J) and R(I, i) are closed forms of
// the grid coordinates (per axis 1.0 at distance 1 of 2J, 0.5 at distance 0 and 2, nothing else).
//
// Order (the same bits as host_setup.cpp: spgemm_csr on the Kronecker operators).  Every weight is
// a product of powers of two, so a * w and r * (A P) are exact and only the order of the additions
// counts.  Entry (i, J) of A P receives a_ik P(k, J) in ascending k (A's row order; a row k of P
// holds J at most once), the first product assigned, the others added; it exists as soon as one k
// of the row has P(k, J) != 0, whatever a_ik is (exact zeros are kept).  Entry (I, J) of R (A P)
// receives R(I, i) (A P)(i, J) in ascending fine index i, first assigned, others added.
//
// Form.  The coarse columns of a fine row are not monotone in k (a row of P spreads over 2^(dim-1)
// coarse lines), so there is no single open accumulator.  Instead one LANE owns one output entry
// (I, J): a group of SLOTS lanes takes coarse row I, finds the box of coarse columns the rows i of
// R's row I can reach (lane s walks fine row i_s, then a min / max butterfly over the group), and
// lane s takes the s-th column of the box in (z, y, x) order -- ascending J, the order of the output
// row.  It then walks the rows i ascending and their entries k ascending and accumulates its own
// entry in registers, A P fused into the R pass.  The lanes of a group read the same entries of A
// (one broadcast load per wave), a fine row is shared by at most 2^dim neighbouring groups, so A is
// streamed from memory once and the only other traffic is the output.  A box of more than SLOTS
// columns (9 of 16 in 2-D, 27 of 32 in 3-D for the 5- / 9- and 7- / 27-point rows) raises *overflow;
// nothing is truncated, the caller takes the host product.
//
// Semi-coarsening (g.cx / cy / cz): on an axis that is not coarsened P1 is the identity -- row k has
// the one column k with weight 1, and R's row I the one fine row I instead of three.
__device__ __forceinline__ void tg_divmod(uint32_t k, uint32_t n, double inv_n, uint32_t* q, uint32_t* r) {
  uint32_t qq = (uint32_t)((double)k * inv_n);  // within 1 of floor(k / n) for k < 2^31
  int32_t rr = (int32_t)(k - qq * n);
  if (rr < 0) { --qq; rr += (int32_t)n; }
  else if ((uint32_t)rr >= n) { ++qq; rr -= (int32_t)n; }
  *q = qq;
  *r = (uint32_t)rr;
}
// coarse columns [l, h] of row k of P1(m): k odd: (k - 1) / 2; k even: k / 2 - 1 and k / 2, inside [0, m)
// (c = 0, the axis is not coarsened: column k alone)
__device__ __forceinline__ void tg_cols(uint32_t k, uint32_t m, uint32_t c, int32_t* l, int32_t* h) {
  if (!c) {
    *l = *h = (int32_t)k;
  } else if (k & 1u) {
    *l = *h = (int32_t)((k - 1u) >> 1);
  } else {
    const int32_t c = (int32_t)(k >> 1);
    *l = c >= 1 ? c - 1 : 0;
    *h = c < (int32_t)m ? c : (int32_t)m - 1;
  }
}
// P1N(k, J) for a column J inside [0, m) on an axis of n fine points; lo / hi: the axis' side bits
__device__ __forceinline__ double tg_weight(uint32_t k, int32_t J, uint32_t c, uint32_t n, uint32_t lo, uint32_t hi) {
  if (!c) return (int32_t)k == J ? 1.0 : 0.0;
  const int32_t t = (int32_t)k - 2 * J;
  if (t == 1) return 1.0;
  if (t == 0) return (lo && J == 0) ? 1.0 : 0.5;
  if (t == 2) return (hi && k + 1u == n) ? 1.0 : 0.5;
  return 0.0;
}
// Periodic axes (PER; host_setup.hpp: tensor_P with periodic).  g.per() holds EVERY periodic axis of
// the level here, coarsened or not: on an axis that is periodic but not coarsened P is the identity,
// yet the wrap entries of A make fine row 0 reach column n - 1, and a min / max box would span the axis.
// So on a periodic axis the reachable columns are kept as offsets d from the group's own coordinate
// C (the fine one where the axis is not coarsened), in the canonical range [-floor(M / 2),
// ceil(M / 2) - 1] of an axis of M columns: a span d_lo .. d_hi then has at most M members, all
// distinct as columns (with M = 2 the left and the right neighbour are one column, one member).  The
// set is the cyclic interval of length len from a = (C + d_lo) mod M; its ascending order is
// [0, a + len - M) then [a, M) when it wraps, so that the lanes of a group still hold the output row
// in ascending flat index.  R's row M - 1 of a coarsened periodic axis has the fine points 0, n - 2,
// n - 1 (ascending) with 0.5, 0.5, 1.0, and row 0 of P the columns 0 and M - 1 with 0.5 each (n >= 4:
// a row of P still holds a column once).  Every wrapped index is a select on an in-range value.
// PER = false is the code without any of this.
__device__ __forceinline__ int32_t tg_delta(int32_t col, int32_t C, int32_t M) {
  const int32_t d = col - C;  // both in [0, M)
  const int32_t e = d < -(M >> 1) ? d + M : d;
  return e > ((M + 1) >> 1) - 1 ? e - M : e;
}
// offsets [l, h] from C of the columns of row k of P1per(2 M) (c = 0: of column k of the identity)
__device__ __forceinline__ void tg_cols_per(uint32_t k, uint32_t m, uint32_t c, uint32_t C, int32_t* l, int32_t* h) {
  if (!c || (k & 1u)) {
    *l = *h = tg_delta((int32_t)(c ? (k - 1u) >> 1 : k), (int32_t)C, (int32_t)m);
  } else {
    const int32_t r = (int32_t)(k >> 1);  // <= m - 1: k <= 2 m - 2
    const int32_t d0 = tg_delta(r >= 1 ? r - 1 : (int32_t)m - 1, (int32_t)C, (int32_t)m);
    const int32_t d1 = tg_delta(r, (int32_t)C, (int32_t)m);
    *l = d0 < d1 ? d0 : d1;
    *h = d0 < d1 ? d1 : d0;
  }
}
// the t-th column (ascending) of the cyclic interval of `len` <= M columns from (C + lo) mod M
__device__ __forceinline__ int32_t tg_lane_col(int32_t t, int32_t lo, int32_t len, int32_t C, int32_t M) {
  const int32_t a0 = C + lo;  // in [-floor(M / 2), 2 M - 2]
  const int32_t a1 = a0 < 0 ? a0 + M : a0;
  const int32_t a = a1 >= M ? a1 - M : a1;
  const int32_t over = a + len - M;  // > 0: the interval wraps, its first `over` members are 0 ..
  return over > 0 ? (t < over ? t : a + t - over) : a + t;
}
// P1per(k, J) for a column J inside [0, m) of a periodic axis (c = 0: the identity)
__device__ __forceinline__ double tg_weight_per(uint32_t k, int32_t J, uint32_t c, uint32_t m) {
  if (!c) return (int32_t)k == J ? 1.0 : 0.0;
  const int32_t t = (int32_t)k - 2 * J;
  if (t == 1) return 1.0;
  if (t == 0 || t == 2) return 0.5;
  return (k == 0u && J + 1 == (int32_t)m) ? 0.5 : 0.0;
}
// the t-th fine point (ascending) of R's row C on a coarsened axis of n points (seam: row n / 2 - 1
// of a periodic axis) and its weight
__device__ __forceinline__ uint32_t tg_fine(uint32_t C, uint32_t t, bool seam) {
  return seam ? (t == 0u ? 0u : 2u * C + t - 1u) : 2u * C + t;
}
template <int SLOTS, bool FILL, bool PER>
__global__ __launch_bounds__(256) void tensor_galerkin_kernel(
    TensorGrid g, double inv_nx, double inv_ny, const int32_t* __restrict__ arp,
    const int32_t* __restrict__ acol, const double* __restrict__ aval, int32_t* __restrict__ cnt,
    const int32_t* __restrict__ orp, int32_t* __restrict__ ocol, double* __restrict__ oval,
    int32_t* __restrict__ overflow) {
  constexpr uint32_t RPB = 256u / SLOTS;  // coarse rows of a workgroup
  const uint32_t nH = g.mx * g.my * g.mz;
  const uint32_t s = threadIdx.x % SLOTS;
  const uint32_t row0 = blockIdx.x * RPB + threadIdx.x / SLOTS;
  const bool live = row0 < nH;
  const uint32_t row = live ? row0 : nH - 1u;  // the tail lanes repeat the last row and write nothing
  const uint32_t I = row % g.mx, qr = row / g.mx, J = qr % g.my, K = qr / g.my;
  const uint32_t rx = g.cx ? 3u : 1u, ry = g.cy ? 3u : 1u, rz = g.cz ? 3u : 1u;
  const uint32_t nt = rx * ry * rz;  // fine rows of R's row, (z, y, x) ascending
  // PER: the periodic axes, and whether this coarse row is the last one of a coarsened periodic axis
  const bool px = PER && (g.per() & 1u), py = PER && (g.per() & 2u), pz = PER && (g.per() & 4u);
  const bool seamx = px && g.cx && 2u * I + 2u == g.nx, seamy = py && g.cy && 2u * J + 2u == g.ny,
             seamz = pz && g.cz && 2u * K + 2u == g.nz;
  // the box of coarse columns (PER: offsets from I / J / K on a periodic axis, which may be negative)
  int32_t lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {-1, -1, -1};
  if (PER) hi[0] = hi[1] = hi[2] = INT32_MIN;
  if (s < nt) {
    const uint32_t ix = g.cx ? tg_fine(I, s % rx, seamx) : I, iy = g.cy ? tg_fine(J, (s / rx) % ry, seamy) : J,
                   iz = g.cz ? tg_fine(K, s / (rx * ry), seamz) : K;
    if (ix < g.nx && iy < g.ny && iz < g.nz) {
      const uint32_t i = (iz * g.ny + iy) * g.nx + ix;
      for (int32_t p = arp[i], e = arp[i + 1]; p < e; ++p) {
        uint32_t kx, ky, kz, q;
        tg_divmod((uint32_t)acol[p], g.nx, inv_nx, &q, &kx);
        tg_divmod(q, g.ny, inv_ny, &kz, &ky);
        int32_t l[3], h[3];
        if (px) tg_cols_per(kx, g.mx, g.cx, I, &l[0], &h[0]);
        else tg_cols(kx, g.mx, g.cx, &l[0], &h[0]);
        if (py) tg_cols_per(ky, g.my, g.cy, J, &l[1], &h[1]);
        else tg_cols(ky, g.my, g.cy, &l[1], &h[1]);
        if (pz) tg_cols_per(kz, g.mz, g.cz, K, &l[2], &h[2]);
        else tg_cols(kz, g.mz, g.cz, &l[2], &h[2]);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          lo[a] = l[a] < lo[a] ? l[a] : lo[a];
          hi[a] = h[a] > hi[a] ? h[a] : hi[a];
        }
      }
    }
  }
#pragma unroll
  for (int d = SLOTS / 2; d >= 1; d >>= 1)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int32_t ol = __shfl_xor(lo[a], d, SLOTS), oh = __shfl_xor(hi[a], d, SLOTS);
      lo[a] = ol < lo[a] ? ol : lo[a];
      hi[a] = oh > hi[a] ? oh : hi[a];
    }
  uint32_t bx = 0, by = 0, vol = 0;
  if (hi[0] >= lo[0]) {  // else: every row of A under this coarse row is empty
    bx = (uint32_t)(hi[0] - lo[0] + 1);
    by = (uint32_t)(hi[1] - lo[1] + 1);
    const uint32_t bz = (uint32_t)(hi[2] - lo[2] + 1);
    if (bx > (uint32_t)SLOTS || by > (uint32_t)SLOTS || bz > (uint32_t)SLOTS || bx * by * bz > (uint32_t)SLOTS) {
      if (s == 0 && live) atomicOr(overflow, 1);
    } else {
      vol = bx * by * bz;
    }
  }
  // this lane's entry (I, J) of R (A P)
  bool hit = false;
  double acc = 0.0;
  int32_t Jx = 0, Jy = 0, Jz = 0;
  if (s < vol) {
    Jx = lo[0] + (int32_t)(s % bx);
    Jy = lo[1] + (int32_t)((s / bx) % by);
    Jz = lo[2] + (int32_t)(s / (bx * by));
    if (px) Jx = tg_lane_col((int32_t)(s % bx), lo[0], (int32_t)bx, (int32_t)I, (int32_t)g.mx);
    if (py) Jy = tg_lane_col((int32_t)((s / bx) % by), lo[1], (int32_t)by, (int32_t)J, (int32_t)g.my);
    if (pz) Jz = tg_lane_col((int32_t)(s / (bx * by)), lo[2], (int32_t)(vol / (bx * by)), (int32_t)K, (int32_t)g.mz);
    for (uint32_t tz = 0; tz < 3; ++tz) {
      if (!g.cz && tz > 0) break;
      const uint32_t iz = g.cz ? tg_fine(K, tz, seamz) : K;
      if (iz >= g.nz) break;
      const double wz = seamz ? (tz == 2u ? 1.0 : 0.5)
                              : (g.cz ? tn_weight<double>(K, tz, g.nz, g.sides & 16u, g.sides & 32u) : 1.0);
      for (uint32_t ty = 0; ty < 3; ++ty) {
        if (!g.cy && ty > 0) break;
        const uint32_t iy = g.cy ? tg_fine(J, ty, seamy) : J;
        if (iy >= g.ny) break;
        const double rzy = wz * (seamy ? (ty == 2u ? 1.0 : 0.5)
                                       : (g.cy ? tn_weight<double>(J, ty, g.ny, g.sides & 4u, g.sides & 8u) : 1.0));
        for (uint32_t tx = 0; tx < 3; ++tx) {
          if (!g.cx && tx > 0) break;
          const uint32_t ix = g.cx ? tg_fine(I, tx, seamx) : I;
          if (ix >= g.nx) break;
          const double r = rzy * (seamx ? (tx == 2u ? 1.0 : 0.5)
                                        : (g.cx ? tn_weight<double>(I, tx, g.nx, g.sides & 1u, g.sides & 2u) : 1.0));  // R(I, i)
          const uint32_t i = (iz * g.ny + iy) * g.nx + ix;
          bool hit_i = false;
          double ap = 0.0;  // (A P)(i, J)
          for (int32_t p = arp[i], e = arp[i + 1]; p < e; ++p) {
            uint32_t kx, ky, kz, q;
            tg_divmod((uint32_t)acol[p], g.nx, inv_nx, &q, &kx);
            tg_divmod(q, g.ny, inv_ny, &kz, &ky);
            const double w = (px ? tg_weight_per(kx, Jx, g.cx, g.mx) : tg_weight(kx, Jx, g.cx, g.nx, g.sides & 1u, g.sides & 2u)) *
                             (py ? tg_weight_per(ky, Jy, g.cy, g.my) : tg_weight(ky, Jy, g.cy, g.ny, g.sides & 4u, g.sides & 8u)) *
                             (pz ? tg_weight_per(kz, Jz, g.cz, g.mz) : tg_weight(kz, Jz, g.cz, g.nz, g.sides & 16u, g.sides & 32u));
            if (w != 0.0) {
              if (FILL) {
                const double t = aval[p] * w;
                ap = hit_i ? ap + t : t;  // first product: assign
              }
              hit_i = true;
            }
          }
          if (hit_i) {
            if (FILL) {
              const double t = r * ap;
              acc = hit ? acc + t : t;
            }
            hit = true;
          }
        }
      }
    }
  }
  const unsigned long long ball = __ballot(hit);
  const uint32_t g0 = ((threadIdx.x & 63u) / SLOTS) * SLOTS;
  const unsigned long long mine = (ball >> g0) & (SLOTS == 64 ? ~0ull : ((1ull << SLOTS) - 1ull));
  if (!FILL) {
    if (s == 0 && live) cnt[row] = (int32_t)__popcll(mine);
  } else if (hit && live) {
    const int32_t at = orp[row] + (int32_t)__popcll(mine & ((1ull << s) - 1ull));
    ocol[at] = (int32_t)(((uint32_t)Jz * g.my + (uint32_t)Jy) * g.mx + (uint32_t)Jx);
    oval[at] = acc;
  }
}
// periodic: the solver's periodic axes.  The kernel needs every one of them, also those this level
// does not coarsen (see above), so the seam bits are set from `periodic`, not `periodic & mask`.
hipError_t launch_tensor_galerkin(bool fill, int dim, const int64_t dims[3], uint32_t mask, uint32_t sides, uint32_t periodic,
                                  const int32_t* arp,
                                  const int32_t* acol, const double* aval, int32_t* cnt,
                                  const int32_t* orp, int32_t* ocol, double* oval, int32_t* overflow,
                                  hipStream_t st) {
  TensorGrid g;
  if (!tensor_grid(dim, dims, mask, sides, periodic, &g)) return hipErrorInvalidValue;
  g.sides = (g.sides & 0xffu) | (periodic << 8);
  const uint32_t nH = g.mx * g.my * g.mz;
  const double inv_nx = 1.0 / (double)g.nx, inv_ny = 1.0 / (double)g.ny;
#define TG_LAUNCH(SLOTS, FILL, PER)                                                                        \
  hipLaunchKernelGGL((tensor_galerkin_kernel<SLOTS, FILL, PER>), dim3((nH + 256u / SLOTS - 1u) / (256u / SLOTS)), \
                     dim3(256), 0, st, g, inv_nx, inv_ny, arp, acol, aval, cnt, orp, ocol, oval, overflow)
  if (periodic) {
    if (dim == 3) {
      if (fill) TG_LAUNCH(32, true, true);
      else TG_LAUNCH(32, false, true);
    } else {
      if (fill) TG_LAUNCH(16, true, true);
      else TG_LAUNCH(16, false, true);
    }
  } else if (dim == 3) {
    if (fill) TG_LAUNCH(32, true, false);
    else TG_LAUNCH(32, false, false);
  } else {
    if (fill) TG_LAUNCH(16, true, false);
    else TG_LAUNCH(16, false, false);
  }
#undef TG_LAUNCH
  return hipGetLastError();
}

// ------------------------------------------------ K-AxisWeights / K-AxisGalerkin ---
// The device set-up of a level that coarsens ONE axis with weights from its own matrix
// (amg_hip_create_tensor_opdep_dev; host_setup.hpp: axis_opdep_P, axis_opdep_row).
//
// K-AxisWeights.  One lane per fine point with an even axis coordinate, i.e. per pair of W: lane e
// of the even-point grid (the level's grid with the axis shortened to mE = m - floor(m / 2), x
// fastest) walks row i of CSR(A_l) in ascending column order and adds each value into s_m, s_0 or
// s_p (from +0.0) by the axis coordinate of its column -- one serial chain per sum, the host's order,
// so the bits are the host's.  One negation and one IEEE division per weight; 0.0 where the neighbour
// does not exist.  A row the host would refuse (s_0 zero or not finite, a weight not finite) sends its
// fine index through atomicMin into *first_bad (INT32_MAX before the launch), as K-CsrCheck does.
// Index arithmetic: 32-bit under the device set-up's guard n < 2^28 (2 e + 1 included), coordinates
// by tg_divmod.
struct AxisSetupGrid {
  uint32_t nx, ny, nz;  // fine
  uint32_t m, mE;       // the axis: fine length, even points m - floor(m / 2)
  uint32_t axis;
  double inv_nx, inv_ny, inv_ex, inv_ey;  // reciprocals of nx, ny and of the even grid's x / y lengths
};
__device__ __forceinline__ uint32_t ax_coord(uint32_t k, const AxisSetupGrid& g) {  // axis coordinate of fine index k
  uint32_t q, kx, ky, kz;
  tg_divmod(k, g.nx, g.inv_nx, &q, &kx);
  if (g.axis == 0u) return kx;
  tg_divmod(q, g.ny, g.inv_ny, &kz, &ky);
  return g.axis == 1u ? ky : kz;
}
// PER: the axis wraps (axis_opdep_row with periodic; m even and >= 4, so mE = m / 2).  The classes of
// the collapse are (c_col - c) mod m = m - 1, 0, 1 -- the wrapped distance is a select on the plain one,
// which lies in (-m, m) -- and every even point has both neighbours: both weights are divided and
// stored whatever their value.  PER = false is the code without the seam.
template <bool PER>
__global__ __launch_bounds__(256) void axis_weights_kernel(AxisSetupGrid g, uint32_t n_even,
                                                           const int32_t* __restrict__ arp,
                                                           const int32_t* __restrict__ acol,
                                                           const double* __restrict__ aval, double* __restrict__ W,
                                                           int32_t* __restrict__ first_bad) {
  const uint32_t e = blockIdx.x * 256u + threadIdx.x;
  if (e >= n_even) return;
  const uint32_t ex = g.axis == 0u ? g.mE : g.nx, ey = g.axis == 1u ? g.mE : g.ny;
  uint32_t q, x, y, z;
  tg_divmod(e, ex, g.inv_ex, &q, &x);
  tg_divmod(q, ey, g.inv_ey, &z, &y);
  const uint32_t c = 2u * (g.axis == 0u ? x : (g.axis == 1u ? y : z));
  const uint32_t i = g.axis == 0u ? (z * g.ny + y) * g.nx + c
                                  : (g.axis == 1u ? (z * g.ny + c) * g.nx + x : (c * g.ny + y) * g.nx + x);
  double sm = 0.0, s0 = 0.0, sp = 0.0;
  for (int32_t p = arp[i], pe = arp[i + 1]; p < pe; ++p) {
    const int32_t d0 = (int32_t)ax_coord((uint32_t)acol[p], g) - (int32_t)c;
    const int32_t dc = PER && d0 < 0 ? d0 + (int32_t)g.m : d0;
    const double v = aval[p];
    if (dc == (PER ? (int32_t)g.m - 1 : -1)) sm += v;
    else if (dc == 0) s0 += v;
    else if (dc == 1) sp += v;
  }
  const bool has_lo = PER || c >= 2u, has_hi = PER || c + 1u < g.m;
  const double wlo = has_lo ? (-sm) / s0 : 0.0;
  const double whi = has_hi ? (-sp) / s0 : 0.0;
  // finite: |x| < inf; a NaN fails the comparison
  const bool bad = s0 == 0.0 || !(fabs(s0) < HUGE_VAL) || !(fabs(wlo) < HUGE_VAL) || !(fabs(whi) < HUGE_VAL);
  if (bad) atomicMin(first_bad, (int32_t)i);
  *reinterpret_cast<double2*>(W + 2u * (size_t)e) = make_double2(wlo, whi);  // W is 16-byte aligned
}
static bool axis_setup_grid(int dim, const int64_t dims[3], int axis, AxisSetupGrid* g, uint32_t* n_even) {
  if ((dim != 2 && dim != 3) || !dims || axis < 0 || axis >= dim) return false;
  const int64_t nx = dims[0], ny = dims[1], nz = dim == 3 ? dims[2] : 1;
  if (nx < 1 || ny < 1 || nz < 1 || (dim == 2 && dims[2] != 1) || dims[axis] < 2) return false;
  if (nx >= ((int64_t)1 << 28) / ny / nz) return false;  // 32-bit indices, 2 e + 1 included
  g->nx = (uint32_t)nx;
  g->ny = (uint32_t)ny;
  g->nz = (uint32_t)nz;
  g->m = (uint32_t)dims[axis];
  g->mE = g->m - g->m / 2u;
  g->axis = (uint32_t)axis;
  const uint32_t ex = axis == 0 ? g->mE : g->nx, ey = axis == 1 ? g->mE : g->ny, ez = axis == 2 ? g->mE : g->nz;
  g->inv_nx = 1.0 / (double)g->nx;
  g->inv_ny = 1.0 / (double)g->ny;
  g->inv_ex = 1.0 / (double)ex;
  g->inv_ey = 1.0 / (double)ey;
  *n_even = ex * ey * ez;
  return true;
}
// periodic: the solver's periodic axes; the seam form runs when `axis` is one of them (even, >= 4)
hipError_t launch_axis_weights(int dim, const int64_t dims[3], int axis, uint32_t periodic, const int32_t* arp,
                               const int32_t* acol, const double* aval, double* W, int32_t* first_bad, hipStream_t st) {
  AxisSetupGrid g;
  uint32_t n_even = 0;
  if (!axis_setup_grid(dim, dims, axis, &g, &n_even) || (reinterpret_cast<uintptr_t>(W) & 15u)) return hipErrorInvalidValue;
  if (periodic >= (1u << dim)) return hipErrorInvalidValue;
  if ((periodic >> axis) & 1u) {
    if (g.m < 4u || (g.m & 1u)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(axis_weights_kernel<true>, dim3((n_even + 255u) / 256u), dim3(256), 0, st, g, n_even, arp, acol, aval,
                       W, first_bad);
  } else {
    hipLaunchKernelGGL(axis_weights_kernel<false>, dim3((n_even + 255u) / 256u), dim3(256), 0, st, g, n_even, arp, acol, aval,
                       W, first_bad);
  }
  return hipGetLastError();
}

// K-AxisGalerkin.  A_H = R (A P) for the one-axis pair with the weights W of K-AxisWeights; the form
// is K-TensorGalerkin's (a group of SLOTS lanes per coarse row, the box of reachable coarse columns
// by a min / max butterfly, lane s owning the s-th column in ascending order, A P fused into the R
// pass in registers, *overflow when a box exceeds the group).  What differs:
//  - P(k, J) along the axis, ck the axis coordinate of k: ck odd: 1.0 at J = (ck - 1) / 2; ck even:
//    W[2 e(k)] at ck / 2 - 1 and W[2 e(k) + 1] at ck / 2, where that coarse point exists; the other
//    coordinates equal.  R(I, i) = P(i, I): fine rows 2 I (w_hi of that point), 2 I + 1 (1.0) and
//    2 I + 2 (w_lo of that point, when < m), ascending for every axis.
//  - The structure is geometric: an entry of P exists for every neighbour that exists, whatever its
//    value (axis_opdep_P keeps 0.0 and -0.0, spgemm_rows keeps an output entry as soon as one stored
//    entry of P is touched), so the hit is "the neighbour exists", never w != 0.0, and a +-0.0 weight
//    still contributes its signed-zero product.
//  - The weights are no powers of two: every product rounds (-ffp-contract=off keeps it apart from
//    the addition).  t = a_ik * P(k, J) for k ascending, first assigned, the rest added; then
//    R(I, i) * (A P)(i, J) for i ascending, first assigned, the rest added -- spgemm_rows' order.
//    The multiplications by 1.0 are done.
// The count pass (FILL = false) reads neither the values nor W.
//
// PER (amg_hip_create_tensor_opdep_periodic_dev): g.per() holds EVERY periodic axis of the solver,
// whether this level coarsens it or not, for K-TensorGalerkin's reason: a wrap entry of A on an axis
// the level leaves alone still makes a min / max box span that axis.  On a periodic axis the reachable
// columns are offsets from the group's own coordinate (tg_cols_per), and lane s takes the s-th column
// of the cyclic interval in ascending flat index (tg_lane_col).  On the coarsened axis, when it wraps
// (m even, >= 4): R's last row H = m / 2 - 1 has the fine points 0, m - 2, m - 1, ascending
// (tg_fine), with W[2 e(0)] (w_lo of fine 0), W[2 e(m - 2) + 1] (w_hi of fine m - 2) and 1.0; every
// row of R has three points; an even ka = 2 q of P has the columns (q - 1) mod (m / 2) (w_lo) and q
// (w_hi), distinct since m / 2 >= 2.  A coarsened axis that does not wrap keeps the rule above bit for
// bit inside a PER launch.  PER = false is the code without any of this.
template <int SLOTS, bool FILL, bool PER>
__global__ __launch_bounds__(256) void axis_galerkin_kernel(
    TensorGrid g, uint32_t axis, uint32_t mE, double inv_nx, double inv_ny, const int32_t* __restrict__ arp,
    const int32_t* __restrict__ acol, const double* __restrict__ aval, const double* __restrict__ W,
    int32_t* __restrict__ cnt, const int32_t* __restrict__ orp, int32_t* __restrict__ ocol,
    double* __restrict__ oval, int32_t* __restrict__ overflow) {
  constexpr uint32_t RPB = 256u / SLOTS;  // coarse rows of a workgroup
  const uint32_t nH = g.mx * g.my * g.mz;
  const uint32_t s = threadIdx.x % SLOTS;
  const uint32_t row0 = blockIdx.x * RPB + threadIdx.x / SLOTS;
  const bool live = row0 < nH;
  const uint32_t row = live ? row0 : nH - 1u;  // the tail lanes repeat the last row and write nothing
  const uint32_t I = row % g.mx, qr = row / g.mx, J = qr % g.my, K = qr / g.my;
  const uint32_t m = axis == 0u ? g.nx : (axis == 1u ? g.ny : g.nz);       // fine length of the axis
  const uint32_t stride = axis == 0u ? 1u : (axis == 1u ? g.nx : g.nx * g.ny);  // of the axis, fine and even grids
  const uint32_t H = axis == 0u ? I : (axis == 1u ? J : K);
  // fine index of R's first row (axis coordinate 2 H) and the even-grid index of that point
  const uint32_t i0 = axis == 0u ? (K * g.ny + J) * g.nx + 2u * I
                                 : (axis == 1u ? (K * g.ny + 2u * J) * g.nx + I : (2u * K * g.ny + J) * g.nx + I);
  const uint32_t e0 = axis == 0u ? (K * g.ny + J) * mE + I : (axis == 1u ? (K * mE + J) * g.nx + I : row);
  // PER: the periodic axes, and whether this coarse row is the last one of the axis when it wraps
  const bool px = PER && (g.per() & 1u), py = PER && (g.per() & 2u), pz = PER && (g.per() & 4u);
  const bool seam = PER && ((g.per() >> axis) & 1u) && 2u * H + 2u == m;
  const uint32_t ib = i0 - 2u * H * stride;  // PER: the fine index with the axis coordinate 0
  const uint32_t nt = 2u * H + 2u < m || seam ? 3u : 2u;  // fine rows of R's row
  int32_t lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {-1, -1, -1};
  if (PER) hi[0] = hi[1] = hi[2] = INT32_MIN;  // offsets may be negative
  if (s < nt) {
    const uint32_t i = PER ? ib + tg_fine(H, s, seam) * stride : i0 + s * stride;
    for (int32_t p = arp[i], e = arp[i + 1]; p < e; ++p) {
      uint32_t kx, ky, kz, q;
      tg_divmod((uint32_t)acol[p], g.nx, inv_nx, &q, &kx);
      tg_divmod(q, g.ny, inv_ny, &kz, &ky);
      int32_t l[3], h[3];
      if (px) tg_cols_per(kx, g.mx, g.cx, I, &l[0], &h[0]);
      else tg_cols(kx, g.mx, g.cx, &l[0], &h[0]);
      if (py) tg_cols_per(ky, g.my, g.cy, J, &l[1], &h[1]);
      else tg_cols(ky, g.my, g.cy, &l[1], &h[1]);
      if (pz) tg_cols_per(kz, g.mz, g.cz, K, &l[2], &h[2]);
      else tg_cols(kz, g.mz, g.cz, &l[2], &h[2]);
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        lo[a] = l[a] < lo[a] ? l[a] : lo[a];
        hi[a] = h[a] > hi[a] ? h[a] : hi[a];
      }
    }
  }
#pragma unroll
  for (int d = SLOTS / 2; d >= 1; d >>= 1)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int32_t ol = __shfl_xor(lo[a], d, SLOTS), oh = __shfl_xor(hi[a], d, SLOTS);
      lo[a] = ol < lo[a] ? ol : lo[a];
      hi[a] = oh > hi[a] ? oh : hi[a];
    }
  uint32_t bx = 0, by = 0, vol = 0;
  if (hi[0] >= lo[0]) {  // else: every row of A under this coarse row is empty
    bx = (uint32_t)(hi[0] - lo[0] + 1);
    by = (uint32_t)(hi[1] - lo[1] + 1);
    const uint32_t bz = (uint32_t)(hi[2] - lo[2] + 1);
    if (bx > (uint32_t)SLOTS || by > (uint32_t)SLOTS || bz > (uint32_t)SLOTS || bx * by * bz > (uint32_t)SLOTS) {
      if (s == 0 && live) atomicOr(overflow, 1);
    } else {
      vol = bx * by * bz;
    }
  }
  // this lane's entry (I, J) of R (A P)
  bool hit = false;
  double acc = 0.0;
  int32_t Jc[3] = {0, 0, 0};
  if (s < vol) {
    Jc[0] = lo[0] + (int32_t)(s % bx);
    Jc[1] = lo[1] + (int32_t)((s / bx) % by);
    Jc[2] = lo[2] + (int32_t)(s / (bx * by));
    if (px) Jc[0] = tg_lane_col((int32_t)(s % bx), lo[0], (int32_t)bx, (int32_t)I, (int32_t)g.mx);
    if (py) Jc[1] = tg_lane_col((int32_t)((s / bx) % by), lo[1], (int32_t)by, (int32_t)J, (int32_t)g.my);
    if (pz) Jc[2] = tg_lane_col((int32_t)(s / (bx * by)), lo[2], (int32_t)(vol / (bx * by)), (int32_t)K, (int32_t)g.mz);
    const int32_t Ja = axis == 0u ? Jc[0] : (axis == 1u ? Jc[1] : Jc[2]);
    const bool pa = PER && ((g.per() >> axis) & 1u);  // the coarsened axis wraps
    for (uint32_t t = 0; t < nt; ++t) {
      const uint32_t i = PER ? ib + tg_fine(H, t, seam) * stride : i0 + t * stride;
      double r = 1.0;  // R(I, i)
      if (PER && seam) {  // fine 0 (its w_lo), fine m - 2 (its w_hi), fine m - 1
        if (FILL && t == 0u) r = W[2u * (e0 - H * stride)];
        if (FILL && t == 1u) r = W[2u * e0 + 1u];
      } else {
        if (FILL && t == 0u) r = W[2u * e0 + 1u];
        if (FILL && t == 2u) r = W[2u * (e0 + stride)];
      }
      bool hit_i = false;
      double ap = 0.0;  // (A P)(i, J)
      for (int32_t p = arp[i], e = arp[i + 1]; p < e; ++p) {
        uint32_t kc[3], q;
        tg_divmod((uint32_t)acol[p], g.nx, inv_nx, &q, &kc[0]);
        tg_divmod(q, g.ny, inv_ny, &kc[2], &kc[1]);
        const uint32_t ka = axis == 0u ? kc[0] : (axis == 1u ? kc[1] : kc[2]);
        // the other coordinates equal; along the axis J is (ka - 1) / 2, or one of ka / 2 - 1, ka / 2
        bool other = true;
#pragma unroll
        for (uint32_t a = 0; a < 3u; ++a) other = other && (a == axis || (int32_t)kc[a] == Jc[a]);
        const int32_t half = (int32_t)(ka >> 1);
        const bool odd = (ka & 1u) != 0u;
        // Ja lies in [0, floor(m / 2)); pa: the low neighbour of ka = 0 is the last coarse point
        const int32_t below = pa && half == 0 ? (int32_t)(m >> 1) - 1 : half - 1;
        const bool at_lo = !odd && Ja == below, at_hi = !odd && Ja == half;
        if (other && ((odd && Ja == half) || at_lo || at_hi)) {
          if (FILL) {
            double w = 1.0;
            if (!odd) {  // even point ka / 2 of the axis, the other coordinates k's own
              const uint32_t ek = axis == 0u ? (kc[2] * g.ny + kc[1]) * mE + (uint32_t)half
                                             : (axis == 1u ? (kc[2] * mE + (uint32_t)half) * g.nx + kc[0]
                                                           : ((uint32_t)half * g.ny + kc[1]) * g.nx + kc[0]);
              w = W[2u * ek + (at_hi ? 1u : 0u)];
            }
            const double tt = aval[p] * w;
            ap = hit_i ? ap + tt : tt;  // first product: assign
          }
          hit_i = true;
        }
      }
      if (hit_i) {
        if (FILL) {
          const double tt = r * ap;
          acc = hit ? acc + tt : tt;
        }
        hit = true;
      }
    }
  }
  const unsigned long long ball = __ballot(hit);
  const uint32_t g0 = ((threadIdx.x & 63u) / SLOTS) * SLOTS;
  const unsigned long long mine = (ball >> g0) & ((1ull << SLOTS) - 1ull);
  if (!FILL) {
    if (s == 0 && live) cnt[row] = (int32_t)__popcll(mine);
  } else if (hit && live) {
    const int32_t at = orp[row] + (int32_t)__popcll(mine & ((1ull << s) - 1ull));
    ocol[at] = (int32_t)(((uint32_t)Jc[2] * g.my + (uint32_t)Jc[1]) * g.mx + (uint32_t)Jc[0]);
    oval[at] = acc;
  }
}
// periodic: the solver's periodic axes.  As in launch_tensor_galerkin the kernel needs every one of
// them, also those this level does not coarsen, so the seam bits are `periodic`, not `periodic & mask`.
hipError_t launch_axis_galerkin(bool fill, int dim, const int64_t dims[3], int axis, uint32_t periodic,
                                const int32_t* arp, const int32_t* acol, const double* aval, const double* W,
                                int32_t* cnt, const int32_t* orp, int32_t* ocol, double* oval, int32_t* overflow,
                                hipStream_t st) {
  TensorGrid g;
  AxisSetupGrid ag;
  uint32_t n_even = 0;
  // tensor_grid: a coarsened periodic axis is even and >= 4
  if (!axis_setup_grid(dim, dims, axis, &ag, &n_even) || !tensor_grid(dim, dims, 1u << axis, 0u, periodic, &g))
    return hipErrorInvalidValue;
  g.sides = periodic << 8;
  const uint32_t nH = g.mx * g.my * g.mz;
#define AG_LAUNCH(SLOTS, FILL, PER)                                                                                    \
  hipLaunchKernelGGL((axis_galerkin_kernel<SLOTS, FILL, PER>), dim3((nH + 256u / SLOTS - 1u) / (256u / SLOTS)), dim3(256), \
                     0, st, g, (uint32_t)axis, ag.mE, ag.inv_nx, ag.inv_ny, arp, acol, aval, W, cnt, orp, ocol, oval, \
                     overflow)
  if (periodic) {
    if (dim == 3) {
      if (fill) AG_LAUNCH(32, true, true);
      else AG_LAUNCH(32, false, true);
    } else {
      if (fill) AG_LAUNCH(16, true, true);
      else AG_LAUNCH(16, false, true);
    }
  } else if (dim == 3) {
    if (fill) AG_LAUNCH(32, true, false);
    else AG_LAUNCH(32, false, false);
  } else {
    if (fill) AG_LAUNCH(16, true, false);
    else AG_LAUNCH(16, false, false);
  }
#undef AG_LAUNCH
  return hipGetLastError();
}

// --------------------------------------------------------------- K-Setup ------
// Setup on the device end to end: the Grid generators
// (grid.hpp:88-98 and the 7-point analogue) as kernels, and the dictionary encoder of the
// level matrices, so that a Poisson hierarchy never exists as host arrays unless a getter
// asks for one.
// A = sum over axes of I (x) .. D .. (x) I, D = tridiag(1, -2, 1) / h^2: row c holds its lower
// neighbours (axes dim-1 .. 0), the diagonal, its upper neighbours (axes 0 .. dim-1) --
// ascending columns, the order host_setup.cpp: laplacian() produces.
// n_last: units (grid lines in 2-D, x-y planes in 3-D) of the slowest axis -- n for the whole
// problem, fewer for the window of a sharded solver (host_setup.cpp: laplacian).
__global__ __launch_bounds__(256) void lap_count_kernel(int dim, int64_t n, int64_t n_last, int64_t N,
                                                        int32_t* __restrict__ cnt) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= N) return;
  const int64_t co[3] = {c % n, dim == 2 ? c / n : (c / n) % n, c / (n * n)};
  const int64_t ext[3] = {n, dim == 2 ? n_last : n, n_last};
  int k = 1;
  for (int a = 0; a < dim; ++a) k += (co[a] > 0) + (co[a] + 1 < ext[a]);
  cnt[c] = k;
}
__global__ __launch_bounds__(256) void lap_fill_kernel(int dim, int64_t n, int64_t n_last, int64_t N,
                                                       const int32_t* __restrict__ rowptr,
                                                       int32_t* __restrict__ col,
                                                       double* __restrict__ val, double off,
                                                       double diag) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= N) return;
  const int64_t co[3] = {c % n, dim == 2 ? c / n : (c / n) % n, c / (n * n)};
  const int64_t ext[3] = {n, dim == 2 ? n_last : n, n_last};
  const int64_t st[3] = {1, n, n * n};
  int64_t p = rowptr[c];
  for (int a = dim - 1; a >= 0; --a)
    if (co[a] > 0) { col[p] = (int32_t)(c - st[a]); val[p] = off; ++p; }
  col[p] = (int32_t)c; val[p] = diag; ++p;
  for (int a = 0; a < dim; ++a)
    if (co[a] + 1 < ext[a]) { col[p] = (int32_t)(c + st[a]); val[p] = off; ++p; }
}
hipError_t launch_laplacian_count(int dim, int64_t n, int64_t n_last, int64_t N, int32_t* cnt, hipStream_t st) {
  hipLaunchKernelGGL(lap_count_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, dim, n, n_last, N, cnt);
  return hipGetLastError();
}
hipError_t launch_laplacian_fill(int dim, int64_t n, int64_t n_last, int64_t N, const int32_t* rowptr, int32_t* col,
                                 double* val, double off, double diag, hipStream_t st) {
  hipLaunchKernelGGL(lap_fill_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, dim, n, n_last, N,
                     rowptr, col, val, off, diag);
  return hipGetLastError();
}

// stats[0] = longest row (entries that are kept), stats[1] = 1 when the matrix is not
// bitwise symmetric, diag[i] = a_ii (0.0 when absent).  prune: exact zeros do not count.
__global__ __launch_bounds__(256) void csr_inspect_kernel(int64_t n, const int32_t* __restrict__ rowptr,
                                                          const int32_t* __restrict__ col,
                                                          const double* __restrict__ val, int prune,
                                                          int32_t* __restrict__ stats,
                                                          double* __restrict__ diag) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  int len = 0;
  double d = 0.0;
  bool asym = false;
  for (int32_t p = rowptr[i]; p < rowptr[i + 1]; ++p) {
    const int32_t j = col[p];
    const double v = val[p];
    if (!prune || v != 0.0) ++len;
    if (j == i) { d = v; continue; }
    // (j, i) must hold the same bits: binary search in row j
    int32_t lo = rowptr[j], hi = rowptr[j + 1] - 1;
    bool found = false;
    while (lo <= hi) {
      const int32_t mid = (lo + hi) >> 1;
      const int32_t cm = col[mid];
      if (cm == (int32_t)i) {
        found = __double_as_longlong(val[mid]) == __double_as_longlong(v);
        break;
      }
      if (cm < (int32_t)i) lo = mid + 1;
      else hi = mid - 1;
    }
    asym = asym || !found;
  }
  if (diag) diag[i] = d;
  atomicMax(&stats[0], len);
  if (asym) atomicOr(&stats[1], 1);
}
hipError_t launch_csr_inspect(int64_t n, const int32_t* rowptr, const int32_t* col, const double* val,
                              bool prune, int32_t* stats, double* diag, hipStream_t st) {
  hipLaunchKernelGGL(csr_inspect_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, rowptr,
                     col, val, prune ? 1 : 0, stats, diag);
  return hipGetLastError();
}

// Dictionary encoder: row r -> `words` 64-bit words of byte codes into the pair table
// (doff, dval: <= 255 entries in LDS), entries in ascending column order, exact zeros skipped
// when prune.  A pair that is not in the table makes the row a FAILURE: its index goes to
// fail[1 + slot] (first 62 of them, fail[0] counts all) and the host, which proposed the
// table from a sample of rows, adds the row's pairs and runs the pass again -- the encoding is
// exact because every row is checked, however the table was guessed.
__global__ __launch_bounds__(256) void dict_encode_kernel(
    int64_t n, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
    const double* __restrict__ val, int prune, const int32_t* __restrict__ doff,
    const double* __restrict__ dval, int ntab, int words, uint64_t* __restrict__ codes,
    int32_t* __restrict__ fail) {
  __shared__ int32_t toff[256];
  __shared__ long long tval[256];
  if ((int)threadIdx.x < ntab) {
    toff[threadIdx.x] = doff[threadIdx.x];
    tval[threadIdx.x] = __double_as_longlong(dval[threadIdx.x]);
  }
  __syncthreads();
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  uint64_t w[2] = {~(uint64_t)0, ~(uint64_t)0};
  int k = 0;
  bool bad = false;
  for (int32_t p = rowptr[r]; p < rowptr[r + 1]; ++p) {
    const double v = val[p];
    if (prune && v == 0.0) continue;
    const int32_t o = (int32_t)((int64_t)col[p] - r);
    const long long vb = __double_as_longlong(v);
    int code = -1;
    for (int t = 0; t < ntab; ++t)
      if (toff[t] == o && tval[t] == vb) { code = t; break; }
    if (code < 0 || k >= 8 * words) { bad = true; break; }
    w[k >> 3] = (w[k >> 3] & ~((uint64_t)0xFF << (8 * (k & 7)))) | ((uint64_t)code << (8 * (k & 7)));
    ++k;
  }
  if (bad) {
    const int32_t slot = atomicAdd(&fail[0], 1);
    if (slot < 62) fail[1 + slot] = (int32_t)r;
    return;
  }
  for (int q = 0; q < words; ++q) codes[r * words + q] = w[q];
}
// second level: code words -> one byte per row into the word table (<= 255 types; a row
// without entries is type 255); unknown words are failures as above
__global__ __launch_bounds__(256) void dict_type_kernel(int64_t n, const uint64_t* __restrict__ codes,
                                                        int words, const uint64_t* __restrict__ rwords,
                                                        int ntypes, uint8_t* __restrict__ rtype,
                                                        int32_t* __restrict__ fail) {
  __shared__ uint64_t tw[512];
  for (int t = threadIdx.x; t < ntypes * words; t += 256) tw[t] = rwords[t];
  __syncthreads();
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const uint64_t a = codes[r * words], b = words == 2 ? codes[r * 2 + 1] : ~(uint64_t)0;
  if (a == ~(uint64_t)0 && b == ~(uint64_t)0) { rtype[r] = 255; return; }
  int ty = -1;
  for (int t = 0; t < ntypes; ++t)
    if (tw[t * words] == a && (words == 1 || tw[t * 2 + 1] == b)) { ty = t; break; }
  if (ty < 0) {
    const int32_t slot = atomicAdd(&fail[0], 1);
    if (slot < 62) fail[1 + slot] = (int32_t)r;
    return;
  }
  rtype[r] = (uint8_t)ty;
}
hipError_t launch_dict_encode(int64_t n, const int32_t* rowptr, const int32_t* col, const double* val,
                              bool prune, const int32_t* doff, const double* dval, int ntab, int words,
                              uint64_t* codes, int32_t* fail, hipStream_t st) {
  if (ntab > 255 || (words != 1 && words != 2)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(dict_encode_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, rowptr,
                     col, val, prune ? 1 : 0, doff, dval, ntab, words, codes, fail);
  return hipGetLastError();
}
hipError_t launch_dict_types(int64_t n, const uint64_t* codes, int words, const uint64_t* rwords,
                             int ntypes, uint8_t* rtype, int32_t* fail, hipStream_t st) {
  if (ntypes > 255 || (words != 1 && words != 2)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(dict_type_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, codes,
                     words, rwords, ntypes, rtype, fail);
  return hipGetLastError();
}

// K-CsrCheck: the argument check of a caller's device CSR arrays (amg_hip_create_tensor_dev).  One lane
// per row; *first_bad (initialised to INT32_MAX) = smallest offending row.  nnz is the caller's
// rowptr[n], read beforehand: a lane reads col only inside [0, nnz), and only when its own pair of
// row pointers lies in that range in ascending order, whatever the other rows hold.
__global__ __launch_bounds__(256) void csr_check_kernel(int64_t n, int64_t nnz, const int32_t* __restrict__ rowptr,
                                                        const int32_t* __restrict__ col,
                                                        int32_t* __restrict__ first_bad) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t a = rowptr[i], b = rowptr[i + 1];
  bool bad = (i == 0 && a != 0) || a < 0 || b < a || b > nnz;
  if (!bad) {
    int64_t prev = -1;
    for (int64_t p = a; p < b; ++p) {
      const int64_t c = col[p];
      if (c <= prev || c >= n) { bad = true; break; }  // c < 0 included: prev starts at -1
      prev = c;
    }
  }
  if (bad) atomicMin(first_bad, (int32_t)i);
}
hipError_t launch_csr_check(int64_t n, int64_t nnz, const int32_t* rowptr, const int32_t* col, int32_t* first_bad,
                            hipStream_t st) {
  hipLaunchKernelGGL(csr_check_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, nnz, rowptr, col,
                     first_bad);
  return hipGetLastError();
}

// ---------------------------------------------------------------- K-SellPack ----
// The panel layouts of upload_mat (SELL-64, or pruned CSR) from a CSR matrix that already sits on
// the device.  Pass 1 (sell_count_kernel), one lane per row, one wave per 64-row panel: kept[r] =
// entries of row r that stay (exact zeros dropped when prune), pslots[p] = 64 * longest kept row of
// panel p (scanned into soff by the caller), stats[0] = longest kept row, stats[1] = 1 when a kept
// entry lies farther than 32767 columns from its row (no 16-bit relative indices), stats[2] = most
// kept entries in a 256-row block (K-CSR's LDS staging).  Pass 2 is sell_fill_kernel or
// csr_compact_kernel, after the caller has chosen the layout by upload_mat's rule.
__global__ __launch_bounds__(256) void sell_count_kernel(int64_t n, const int32_t* __restrict__ rowptr,
                                                         const int32_t* __restrict__ col,
                                                         const double* __restrict__ val, int prune,
                                                         int32_t* __restrict__ kept, int32_t* __restrict__ pslots,
                                                         int32_t* __restrict__ stats) {
  __shared__ int32_t wsum[4];
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int len = 0;
  bool far = false;
  if (r < n) {
    for (int32_t p = rowptr[r]; p < rowptr[r + 1]; ++p) {
      if (prune && val[p] == 0.0) continue;
      ++len;
      const int64_t d = (int64_t)col[p] - r;
      far = far || d < -32767 || d > 32767;
    }
    kept[r] = len;
  }
  int w = len, sum = len;
  for (int o = 32; o > 0; o >>= 1) {  // every lane of the wave is here: rows past n count 0
    w = max(w, __shfl_xor(w, o, 64));
    sum += __shfl_xor(sum, o, 64);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    wsum[wave] = sum;
    const int64_t p = (int64_t)blockIdx.x * 4 + wave;
    if (p * 64 < n) {
      pslots[p] = w * 64;
      atomicMax(&stats[0], w);
    }
  }
  if (far) atomicOr(&stats[1], 1);
  __syncthreads();
  if (threadIdx.x == 0) atomicMax(&stats[2], wsum[0] + wsum[1] + wsum[2] + wsum[3]);
}
__global__ __launch_bounds__(256) void sell_soff_kernel(int64_t np1, const int32_t* __restrict__ off32,
                                                        int64_t* __restrict__ soff) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p < np1) soff[p] = off32[p];
}
// One lane per row, the padding rows of the last panel included: for every j the wave stores 64
// consecutive slots (base + j * 64) and reads its rows with a stride of one row.
template <bool IDX16>
__global__ __launch_bounds__(256) void sell_fill_kernel(int64_t n, const int32_t* __restrict__ rowptr,
                                                        const int32_t* __restrict__ col,
                                                        const double* __restrict__ val, int prune,
                                                        const int64_t* __restrict__ soff, void* __restrict__ scol,
                                                        double* __restrict__ sval) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t p = r >> 6;
  if (p * 64 >= n) return;
  const int64_t base = soff[p] + (r & 63);
  const int64_t w = (soff[p + 1] - soff[p]) >> 6;
  int16_t* c16 = reinterpret_cast<int16_t*>(scol);
  int32_t* c32 = reinterpret_cast<int32_t*>(scol);
  int64_t j = 0;
  if (r < n) {
    for (int32_t q = rowptr[r]; q < rowptr[r + 1] && j < w; ++q) {
      const double v = val[q];
      if (prune && v == 0.0) continue;
      const int32_t c = col[q];
      if (IDX16) c16[base + j * 64] = (int16_t)((int64_t)c - r);
      else c32[base + j * 64] = c;
      sval[base + j * 64] = v;
      ++j;
    }
  }
  for (; j < w; ++j) {
    if (IDX16) c16[base + j * 64] = (int16_t)-32768;
    else c32[base + j * 64] = -1;
    sval[base + j * 64] = 0.0;
  }
}
// optr = exclusive scan of kept: row r's kept entries in their order
__global__ __launch_bounds__(256) void csr_compact_kernel(int64_t n, const int32_t* __restrict__ rowptr,
                                                          const int32_t* __restrict__ col,
                                                          const double* __restrict__ val, int prune,
                                                          const int32_t* __restrict__ optr, int32_t* __restrict__ ocol,
                                                          double* __restrict__ oval) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  int32_t o = optr[r];
  const int32_t oe = optr[r + 1];
  for (int32_t q = rowptr[r]; q < rowptr[r + 1] && o < oe; ++q) {
    const double v = val[q];
    if (prune && v == 0.0) continue;
    ocol[o] = col[q];
    oval[o] = v;
    ++o;
  }
}
hipError_t launch_sell_count(int64_t n, const int32_t* rowptr, const int32_t* col, const double* val, bool prune,
                             int32_t* kept, int32_t* pslots, int32_t* stats, hipStream_t st) {
  hipLaunchKernelGGL(sell_count_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, rowptr, col, val,
                     prune ? 1 : 0, kept, pslots, stats);
  return hipGetLastError();
}
hipError_t launch_sell_fill(int64_t n, const int32_t* rowptr, const int32_t* col, const double* val, bool prune,
                            const int32_t* off32, int64_t* soff, bool idx16, void* scol, double* sval,
                            hipStream_t st) {
  const int64_t np = (n + 63) / 64;
  hipLaunchKernelGGL(sell_soff_kernel, dim3((unsigned)((np + 1 + 255) / 256)), dim3(256), 0, st, np + 1, off32, soff);
  const unsigned grid = (unsigned)((np * 64 + 255) / 256);
  if (idx16)
    hipLaunchKernelGGL(sell_fill_kernel<true>, dim3(grid), dim3(256), 0, st, n, rowptr, col, val, prune ? 1 : 0, soff,
                       scol, sval);
  else
    hipLaunchKernelGGL(sell_fill_kernel<false>, dim3(grid), dim3(256), 0, st, n, rowptr, col, val, prune ? 1 : 0, soff,
                       scol, sval);
  return hipGetLastError();
}
hipError_t launch_csr_compact(int64_t n, const int32_t* rowptr, const int32_t* col, const double* val, bool prune,
                              const int32_t* optr, int32_t* ocol, double* oval, hipStream_t st) {
  hipLaunchKernelGGL(csr_compact_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, rowptr, col, val,
                     prune ? 1 : 0, optr, ocol, oval);
  return hipGetLastError();
}

// --------------------------------------------------------------- K-Transpose ----
// CSR(A) -> CSC(A) of a square matrix on the device: count per column (atomicAdd), scan (the
// caller), scatter through per-column cursors, then one lane per column sorts its entries by row
// index, which makes the result that of the host transpose whatever order the atomics ran in (row
// indices are unique inside a column).  The sort is a serial insertion sort per lane, meant for
// stencil-sized columns: a column of more than TRANSPOSE_MAX_COL entries sets *overflow and is
// left alone; the caller then discards the result and transposes on the host.
__global__ __launch_bounds__(256) void transpose_count_kernel(int64_t nnz, const int32_t* __restrict__ col,
                                                              int32_t* __restrict__ cnt) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p < nnz) atomicAdd(&cnt[col[p]], 1);
}
__global__ __launch_bounds__(256) void transpose_scatter_kernel(int64_t n, const int32_t* __restrict__ rowptr,
                                                                const int32_t* __restrict__ col,
                                                                const double* __restrict__ val,
                                                                const int32_t* __restrict__ cptr,
                                                                int32_t* __restrict__ cursor,
                                                                int32_t* __restrict__ orow, double* __restrict__ oval) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  for (int32_t p = rowptr[r]; p < rowptr[r + 1]; ++p) {
    const int32_t c = col[p];
    const int32_t q = cptr[c] + atomicAdd(&cursor[c], 1);
    if (q < cptr[c + 1]) {  // always, when cptr is the scan of this matrix's column counts
      orow[q] = (int32_t)r;
      oval[q] = val[p];
    }
  }
}
__global__ __launch_bounds__(256) void transpose_sort_kernel(int64_t n, const int32_t* __restrict__ cptr,
                                                             int32_t* __restrict__ orow, double* __restrict__ oval,
                                                             int32_t* __restrict__ overflow) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= n) return;
  const int32_t s = cptr[c];
  const int len = cptr[c + 1] - s;
  if (len > TRANSPOSE_MAX_COL) {
    atomicOr(overflow, 1);
    return;
  }
  for (int a = 1; a < len; ++a) {  // insertion sort in place: the scatter leaves columns nearly sorted
    const int32_t kr = orow[s + a];
    const double kv = oval[s + a];
    int b = a - 1;
    while (b >= 0 && orow[s + b] > kr) {
      orow[s + b + 1] = orow[s + b];
      oval[s + b + 1] = oval[s + b];
      --b;
    }
    orow[s + b + 1] = kr;
    oval[s + b + 1] = kv;
  }
}
hipError_t launch_transpose_count(int64_t nnz, const int32_t* col, int32_t* cnt, hipStream_t st) {
  if (nnz <= 0) return hipSuccess;
  hipLaunchKernelGGL(transpose_count_kernel, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, st, nnz, col, cnt);
  return hipGetLastError();
}
hipError_t launch_transpose_fill(int64_t n, const int32_t* rowptr, const int32_t* col, const double* val,
                                 const int32_t* cptr, int32_t* cursor, int32_t* orow, double* oval, int32_t* overflow,
                                 hipStream_t st) {
  const unsigned grid = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(transpose_scatter_kernel, dim3(grid), dim3(256), 0, st, n, rowptr, col, val, cptr, cursor, orow,
                     oval);
  hipLaunchKernelGGL(transpose_sort_kernel, dim3(grid), dim3(256), 0, st, n, cptr, orow, oval, overflow);
  return hipGetLastError();
}

// ------------------------------------------------------------------ K-Block ----
// Multi-right-hand-side (block) forms of the V-cycle's row kernels (solver.cpp: "block cycle").
// Vectors are ROW-major panels of n x KP doubles (entry (i, j) at i * KP + j), KP a power of two
// <= 16.  Lane = (row, column): KP consecutive lanes share one row, load the same col / val (the
// same-address loads are served once) and each gathers x[c * KP + j]: a row group reads one
// contiguous 8 KP-byte segment and stores out[row * KP + j] coalesced.  Per (row, column) the
// operations and their order are csr_stage_kernel's (ascending column order, the diagonal picked
// out of the walk for the Jacobi / Chebyshev quotient, the residual's sum started at f), so column
// j has the bits of the single-vector kernel on column j.  KP = 1 is plain thread-per-row CSR.
template <int MODE, int KP>
__global__ __launch_bounds__(256) void block_csr_kernel(
    int64_t n, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
    const double* __restrict__ val, const double* __restrict__ x, const double* f,  // f may be out
    double* out, double omega, double* dvec, double alpha) {
  constexpr int RPB = 256 / KP;  // rows per workgroup
  const int tid = threadIdx.x;
  const int64_t row = (int64_t)blockIdx.x * RPB + tid / KP;
  const int j = tid % KP;
  if (row >= n) return;
  const int64_t o = row * KP + j;
  const int32_t rs = rowptr[row], re = rowptr[row + 1];
  double fi = 0.0, xi = 0.0, di = 0.0;
  if (MODE != CSR_SPMV) fi = f[o];
  if (mode_jac(MODE)) xi = x[o];
  if (mode_cheb(MODE) && !cheb_first(MODE)) di = dvec[o];
  double acc = (MODE == CSR_RESID) ? fi : 0.0;
  double diag = 0.0;
  constexpr int U = 4;  // gathers issued together; the sum itself stays in row order
  for (int32_t p = rs; p < re; p += U) {
    int32_t c[U];
    double v[U], xx[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int32_t q = p + u < re ? p + u : p;
      c[u] = col[q];
      v[u] = val[q];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) xx[u] = x[(int64_t)c[u] * KP + j];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (p + u < re) {
        if (MODE == CSR_RESID) {
          acc -= v[u] * xx[u];
        } else if (mode_jac(MODE)) {
          if ((int64_t)c[u] == row) diag = v[u];
          else acc += v[u] * xx[u];
        } else {
          acc += v[u] * xx[u];
        }
      }
    }
  }
  if (MODE == CSR_RESID || MODE == CSR_SPMV) {
    out[o] = acc;
  } else if (MODE == CSR_SPMV_ADD) {
    out[o] = fi + acc;
  } else if (MODE == CSR_JACOBI) {
    out[o] = (diag == 0.0) ? xi : xi + omega * ((fi - acc) / diag - xi);
  } else if (mode_cheb(MODE)) {
    double dn;
    out[o] = cheb_update<MODE>((diag == 0.0) ? xi : (fi - acc) / diag, xi, di, alpha, omega, dn);
    if (!cheb_last(MODE)) dvec[o] = dn;
  } else {  // CSR_RSSQ
    const double d = fi - acc;
    out[o] = d * d;
  }
}

template <int MODE>
static hipError_t launch_block_csr_m(int kp, int64_t n, const int32_t* rowptr, const int32_t* col,
                                     const double* val, const double* x, const double* f, double* out,
                                     double omega, double* dvec, double alpha, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  const int64_t rpb = 256 / kp;
  const dim3 grid((unsigned)((n + rpb - 1) / rpb));
#define AMG_BLOCK_CSR(KP)                                                                                \
  hipLaunchKernelGGL((block_csr_kernel<MODE, KP>), grid, dim3(256), 0, st, n, rowptr, col, val, x, f, out, \
                     omega, dvec, alpha)
  switch (kp) {
    case 1: AMG_BLOCK_CSR(1); break;
    case 2: AMG_BLOCK_CSR(2); break;
    case 4: AMG_BLOCK_CSR(4); break;
    case 8: AMG_BLOCK_CSR(8); break;
    case 16: AMG_BLOCK_CSR(16); break;
    default: return hipErrorInvalidValue;
  }
#undef AMG_BLOCK_CSR
  return hipGetLastError();
}
hipError_t launch_block_csr(int mode, int kp, int64_t n, const int32_t* rowptr, const int32_t* col,
                            const double* val, const double* x, const double* f, double* out, double omega,
                            hipStream_t st) {
  switch (mode) {
    case CSR_RESID: return launch_block_csr_m<CSR_RESID>(kp, n, rowptr, col, val, x, f, out, omega, nullptr, 0.0, st);
    case CSR_JACOBI: return launch_block_csr_m<CSR_JACOBI>(kp, n, rowptr, col, val, x, f, out, omega, nullptr, 0.0, st);
    case CSR_SPMV: return launch_block_csr_m<CSR_SPMV>(kp, n, rowptr, col, val, x, f, out, omega, nullptr, 0.0, st);
    case CSR_RSSQ: return launch_block_csr_m<CSR_RSSQ>(kp, n, rowptr, col, val, x, f, out, omega, nullptr, 0.0, st);
    case CSR_SPMV_ADD:
      return launch_block_csr_m<CSR_SPMV_ADD>(kp, n, rowptr, col, val, x, f, out, omega, nullptr, 0.0, st);
  }
  return hipErrorInvalidValue;
}
hipError_t launch_block_csr_cheb(int kp, int64_t n, const int32_t* rowptr, const int32_t* col, const double* val,
                                 const double* x, const double* f, double* out, const ChebStep& c, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (!c.d || x == out) return hipErrorInvalidValue;
#define AMG_BLOCK_CHEB(FI, LA)                                                                                 \
  return launch_block_csr_m<cheb_kernel_mode(FI, LA)>(kp, n, rowptr, col, val, x, f, out, c.beta, c.d, c.alpha, \
                                                      st)
  if (c.first && c.last) AMG_BLOCK_CHEB(true, true);
  if (c.first) AMG_BLOCK_CHEB(true, false);
  if (c.last) AMG_BLOCK_CHEB(false, true);
  AMG_BLOCK_CHEB(false, false);
#undef AMG_BLOCK_CHEB
}

// Element-wise block kernels: one lane per panel entry e = i * kp + j (kp = 1 << ks).
static inline dim3 block_grid(int64_t count) { return dim3((unsigned)((count + 255) / 256)); }

// linear_restrict_kernel per column: f_H = ((0 + 0.5 r[2i]) + 1.0 r[2i+1]) + 0.5 r[2i+2]; uH zeroed
__global__ __launch_bounds__(256) void block_restrict_kernel(int64_t n_h, int64_t n_H, int ks,
                                                             const double* __restrict__ r,
                                                             double* __restrict__ fH, double* __restrict__ uH) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (n_H << ks)) return;
  const int64_t jr = e >> ks, c = e & ((1 << ks) - 1);
  if (uH) uH[e] = 0.0;
  const int64_t i = 2 * jr;
  double s = 0.0;
  if (i < n_h) s += 0.5 * r[(i << ks) + c];
  if (i + 1 < n_h) s += 1.0 * r[((i + 1) << ks) + c];
  if (i + 2 < n_h) s += 0.5 * r[((i + 2) << ks) + c];
  fH[e] = s;
}
hipError_t launch_block_restrict(int kp, int64_t n_h, int64_t n_H, const double* r, double* fH, double* uH_zero,
                                 hipStream_t st) {
  if (n_H <= 0) return hipSuccess;
  const int ks = __builtin_ctz((unsigned)kp);
  hipLaunchKernelGGL(block_restrict_kernel, block_grid(n_H * kp), dim3(256), 0, st, n_h, n_H, ks, r, fH, uH_zero);
  return hipGetLastError();
}
// linear_prolong_add2_kernel per column: u_h = u_h + t, t = P u_H (t[2j+1] = 0 + 1.0 u_H[j],
// t[2j] = (0 + 0.5 u_H[j-1]) + 0.5 u_H[j])
__global__ __launch_bounds__(256) void block_prolong_add_kernel(int64_t n_h, int64_t n_H, int ks,
                                                                const double* __restrict__ uH, double* uh) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (n_h << ks)) return;
  const int64_t i = e >> ks, c = e & ((1 << ks) - 1);
  const int64_t j = i >> 1;
  double t = 0.0;
  if (i & 1) {
    if (j < n_H) t += 1.0 * uH[(j << ks) + c];
  } else {
    if (j >= 1 && j - 1 < n_H) t += 0.5 * uH[((j - 1) << ks) + c];
    if (j < n_H) t += 0.5 * uH[(j << ks) + c];
  }
  uh[e] = uh[e] + t;
}
hipError_t launch_block_prolong_add(int kp, int64_t n_h, int64_t n_H, const double* uH, double* uh,
                                    hipStream_t st) {
  if (n_h <= 0) return hipSuccess;
  const int ks = __builtin_ctz((unsigned)kp);
  hipLaunchKernelGGL(block_prolong_add_kernel, block_grid(n_h * kp), dim3(256), 0, st, n_h, n_H, ks, uH, uh);
  return hipGetLastError();
}

// user pitch k <-> internal pitch kp: to_panel pads columns k .. kp-1 with zeros
__global__ __launch_bounds__(256) void block_pitch_kernel(int64_t n, int k, int ks, const double* __restrict__ src,
                                                          double* __restrict__ dst, int to_panel) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (to_panel) {
    if (e >= (n << ks)) return;
    const int64_t i = e >> ks;
    const int c = (int)(e & ((1 << ks) - 1));
    dst[e] = c < k ? src[i * k + c] : 0.0;
  } else {
    if (e >= n * k) return;
    const int64_t i = e / k;
    const int c = (int)(e - i * k);
    dst[e] = src[(i << ks) + c];
  }
}
hipError_t launch_block_pitch(int64_t n, int k, int kp, const double* src, double* dst, bool to_panel,
                              hipStream_t st) {
  if (n <= 0) return hipSuccess;
  const int ks = __builtin_ctz((unsigned)kp);
  hipLaunchKernelGGL(block_pitch_kernel, block_grid(to_panel ? n * kp : n * k), dim3(256), 0, st, n, k, ks, src,
                     dst, to_panel ? 1 : 0);
  return hipGetLastError();
}
// panel (n x kp, row-major) <-> kp contiguous columns of n (the coarse solve's operands)
__global__ __launch_bounds__(256) void block_columns_kernel(int64_t n, int ks, const double* __restrict__ src,
                                                            double* __restrict__ dst, int to_columns) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (n << ks)) return;
  const int64_t i = e >> ks, c = e & ((1 << ks) - 1);
  if (to_columns) dst[c * n + i] = src[e];
  else dst[e] = src[c * n + i];
}
hipError_t launch_block_columns(int kp, int64_t n, const double* src, double* dst, bool to_columns,
                                hipStream_t st) {
  if (n <= 0) return hipSuccess;
  const int ks = __builtin_ctz((unsigned)kp);
  hipLaunchKernelGGL(block_columns_kernel, block_grid(n * kp), dim3(256), 0, st, n, ks, src, dst,
                     to_columns ? 1 : 0);
  return hipGetLastError();
}

// K-SumSq per column: the thread owning rows i, i + G, ... (G = grid x 256) keeps one partial per
// column (s += x, or s += x * y), reading each row's KP contiguous values once; then per column
// the same wave_sum and four-wave combine as sum_kernel / dot_kernel.  Launched with one workgroup
// over the (blocks x KP) partials it is the second stage: sum_kernel's on every column.
template <int KP>
__global__ __launch_bounds__(256) void block_sum_kernel(int64_t n, const double* __restrict__ x,
                                                        const double* __restrict__ y, double* __restrict__ out) {
  __shared__ double part[4][KP];
  double s[KP];
#pragma unroll
  for (int j = 0; j < KP; ++j) s[j] = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
#pragma unroll
    for (int j = 0; j < KP; ++j) {
      const double v = x[i * KP + j];
      s[j] += y ? v * y[i * KP + j] : v;
    }
  }
#pragma unroll
  for (int j = 0; j < KP; ++j) {
    const double w = wave_sum(s[j]);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][j] = w;
  }
  __syncthreads();
  if (threadIdx.x < KP) {
    const int j = threadIdx.x;
    out[(int64_t)blockIdx.x * KP + j] = ((part[0][j] + part[1][j]) + part[2][j]) + part[3][j];
  }
}
// out[j] = sum_i x[i, j] (y == null) or sum_i x[i, j] y[i, j]; scratch: 1024 x kp doubles
hipError_t launch_block_sum(int kp, int64_t n, const double* x, const double* y, double* out, double* scratch,
                            hipStream_t st) {
  int64_t g = (n + 255) / 256;
  if (g > 1024) g = 1024;
  if (g < 1) g = 1;
#define AMG_BLOCK_SUM(KP)                                                                                    \
  hipLaunchKernelGGL(block_sum_kernel<KP>, dim3((unsigned)g), dim3(256), 0, st, n, x, y, scratch);          \
  hipLaunchKernelGGL(block_sum_kernel<KP>, dim3(1), dim3(256), 0, st, g, scratch, (const double*)nullptr, out)
  switch (kp) {
    case 1: AMG_BLOCK_SUM(1); break;
    case 2: AMG_BLOCK_SUM(2); break;
    case 4: AMG_BLOCK_SUM(4); break;
    case 8: AMG_BLOCK_SUM(8); break;
    case 16: AMG_BLOCK_SUM(16); break;
    default: return hipErrorInvalidValue;
  }
#undef AMG_BLOCK_SUM
  return hipGetLastError();
}

// K-PCG per column with a mask: columns whose act[j] is 0 are frozen (x, r, p untouched)
__global__ __launch_bounds__(256) void block_pcg_xr_kernel(int64_t n, int ks, const double* __restrict__ num,
                                                           const double* __restrict__ den,
                                                           const int32_t* __restrict__ act, double* x, double* r,
                                                           const double* __restrict__ p,
                                                           const double* __restrict__ q) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (n << ks)) return;
  const int c = (int)(e & ((1 << ks) - 1));
  if (!act[c]) return;
  const double alpha = num[c] / den[c];
  x[e] = x[e] + alpha * p[e];
  r[e] = r[e] - alpha * q[e];
}
__global__ __launch_bounds__(256) void block_pcg_p_kernel(int64_t n, int ks, const double* __restrict__ num,
                                                          const double* __restrict__ den,
                                                          const int32_t* __restrict__ act, double* p,
                                                          const double* __restrict__ z) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (n << ks)) return;
  const int c = (int)(e & ((1 << ks) - 1));
  if (!act[c]) return;
  const double beta = num[c] / den[c];
  p[e] = z[e] + beta * p[e];
}
hipError_t launch_block_pcg_update_xr(int kp, int64_t n, const double* num, const double* den, const int32_t* act,
                                      double* x, double* r, const double* p, const double* q, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  const int ks = __builtin_ctz((unsigned)kp);
  hipLaunchKernelGGL(block_pcg_xr_kernel, block_grid(n * kp), dim3(256), 0, st, n, ks, num, den, act, x, r, p, q);
  return hipGetLastError();
}
hipError_t launch_block_pcg_update_p(int kp, int64_t n, const double* num, const double* den, const int32_t* act,
                                     double* p, const double* z, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  const int ks = __builtin_ctz((unsigned)kp);
  hipLaunchKernelGGL(block_pcg_p_kernel, block_grid(n * kp), dim3(256), 0, st, n, ks, num, den, act, p, z);
  return hipGetLastError();
}

// K-Center per column of a panel: m_j = sums[j] / (double)n from launch_block_sum's device scalars.
// The panels are allocations of the block path's own, so a row of kp >= 2 contiguous columns starts on
// a 16-byte boundary and a lane takes two columns of one row per access.
// block_center_kernel: v = centre(v) in every column.
template <bool PAIRS>
__global__ __launch_bounds__(256) void block_center_kernel(int64_t n, int ks, const double* __restrict__ sums,
                                                           double* v) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const double dn = (double)n;
  if (PAIRS) {
    if (t >= ((n << ks) >> 1)) return;
    const int c = (int)((2 * t) & ((1 << ks) - 1));
    double2 w = reinterpret_cast<double2*>(v)[t];
    w.x = w.x - sums[c] / dn;
    w.y = w.y - sums[c + 1] / dn;
    reinterpret_cast<double2*>(v)[t] = w;
  } else {
    if (t >= (n << ks)) return;
    v[t] = v[t] - sums[t & ((1 << ks) - 1)] / dn;
  }
}
hipError_t launch_block_center(int kp, int64_t n, const double* sums, double* v, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (((uintptr_t)v & 15) != 0) return hipErrorInvalidValue;
  const int ks = __builtin_ctz((unsigned)kp);
  if (kp >= 2)
    hipLaunchKernelGGL(block_center_kernel<true>, block_grid(n * kp / 2), dim3(256), 0, st, n, ks, sums, v);
  else
    hipLaunchKernelGGL(block_center_kernel<false>, block_grid(n), dim3(256), 0, st, n, ks, sums, v);
  return hipGetLastError();
}
// block_center_dot_kernel<KP>: center_dot_kernel on every column: block_sum_kernel<KP>'s rows per
// thread, order and tree with the term r[i, j] * (z[i, j] - m_j), z stored centred.
template <int KP>
__global__ __launch_bounds__(256) void block_center_dot_kernel(int64_t n, const double* __restrict__ sums,
                                                               double* __restrict__ z, const double* __restrict__ r,
                                                               double* __restrict__ out) {
  __shared__ double part[4][KP];
  double s[KP], m[KP];
#pragma unroll
  for (int j = 0; j < KP; ++j) {
    s[j] = 0.0;
    m[j] = sums[j] / (double)n;
  }
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    if (KP >= 2) {
      double2* zr = reinterpret_cast<double2*>(z + i * KP);
      const double2* rr = reinterpret_cast<const double2*>(r + i * KP);
#pragma unroll
      for (int j = 0; j < KP / 2; ++j) {
        double2 zc = zr[j];
        const double2 rv = rr[j];
        zc.x = zc.x - m[2 * j];
        zc.y = zc.y - m[2 * j + 1];
        zr[j] = zc;
        s[2 * j] += rv.x * zc.x;
        s[2 * j + 1] += rv.y * zc.y;
      }
    } else {
      const double zc = z[i] - m[0];
      z[i] = zc;
      s[0] += r[i] * zc;
    }
  }
#pragma unroll
  for (int j = 0; j < KP; ++j) {
    const double w = wave_sum(s[j]);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][j] = w;
  }
  __syncthreads();
  if (threadIdx.x < KP) {
    const int j = threadIdx.x;
    out[(int64_t)blockIdx.x * KP + j] = ((part[0][j] + part[1][j]) + part[2][j]) + part[3][j];
  }
}
// z = centre(z) per column and out[j] = sum_i r[i, j] z[i, j] of the centred z; scratch: 1024 x kp doubles
hipError_t launch_block_center_dot(int kp, int64_t n, const double* sums, double* z, const double* r, double* out,
                                   double* scratch, hipStream_t st) {
  if ((((uintptr_t)z | (uintptr_t)r) & 15) != 0) return hipErrorInvalidValue;
  int64_t g = (n + 255) / 256;
  if (g > 1024) g = 1024;
  if (g < 1) g = 1;
#define AMG_BLOCK_CENTER_DOT(KP)                                                                                  \
  hipLaunchKernelGGL(block_center_dot_kernel<KP>, dim3((unsigned)g), dim3(256), 0, st, n, sums, z, r, scratch);  \
  hipLaunchKernelGGL(block_sum_kernel<KP>, dim3(1), dim3(256), 0, st, g, scratch, (const double*)nullptr, out)
  switch (kp) {
    case 1: AMG_BLOCK_CENTER_DOT(1); break;
    case 2: AMG_BLOCK_CENTER_DOT(2); break;
    case 4: AMG_BLOCK_CENTER_DOT(4); break;
    case 8: AMG_BLOCK_CENTER_DOT(8); break;
    case 16: AMG_BLOCK_CENTER_DOT(16); break;
    default: return hipErrorInvalidValue;
  }
#undef AMG_BLOCK_CENTER_DOT
  return hipGetLastError();
}

// ---- K-Line: line-relaxation smoother (kernels.hpp: LineRef) -----------------------------------
// T = the entries of A at column offsets 0, +s, -s.  Row i sits on chain c = i % s at position
// p = i / s.  Every chain is cut with period LINE_SEG: positions 32 g .. 32 g + 30 are the interior
// rows of segment g, position 32 g + 31 is a separator.  With the separators removed the segments
// are independent tridiagonal blocks B_g; the Schur complement S on the separators of one chain is
// tridiagonal again.  Setup factors every B_g and S (Thomas, no pivoting) and stores
// v = B_g^-1 (dl_first e_first), w = B_g^-1 (du_last e_last).  One solve is
//   line_seg_kernel     y_g = B_g^-1 r_g                                  lane per (segment, chain)
//   line_sep_*_kernel   S x_s = r_s - dl_s y_(s-1) - du_s y_(s+1)         lane or workgroup per chain
//   line_update_kernel  x = y - v x_(sep before) - w x_(sep after); u += omega x   lane per row
// so the dependent depth is 2 * 31 + 2 * (chain length / 32) steps instead of 2 * chain length.
// Arrays (n doubles each), interior row | separator row:
//   dl: a_(i,i-s) | a_(i,i-s)     ip: 1 / pivot of B_g | 1 / pivot of S     cp: upper / pivot, both
//   v:  v | lower entry of S      w:  w | a_(i,i+s)
namespace {
constexpr int LINE_INT = LINE_SEG - 1;  // interior rows of a full segment

__host__ __device__ inline bool line_bad_pivot(double p) { return !(p == p) || p == 0.0 || p - p != 0.0; }

// a_ij from the CSR rows, 0 when absent
__host__ __device__ inline double line_entry(const int32_t* rowptr, const int32_t* col, const double* val, int64_t i,
                                             int64_t j) {
  for (int32_t p = rowptr[i]; p < rowptr[i + 1]; ++p)
    if (col[p] == j) return val[p];
  return 0.0;
}
// Cyclic lines (kernels.hpp: SeamRef).  The line of row i has stride s and m >= 3 rows, first row i0,
// last row i1; alpha = a(i0, i1) and beta = a(i1, i0) are its wrap entries, gamma = -a(i0, i0).
// Row i of T' = the open row with the diagonal d(i0) - gamma on the first and d(i1) - alpha beta /
// gamma on the last row of the line; transposed: row i of T'^T (its lower entry is the upper entry
// of the row before, its upper entry the lower entry of the row after).
__host__ __device__ inline void line_cyclic_row(int64_t i, int64_t s, int64_t m, const int32_t* rowptr,
                                                const int32_t* col, const double* val, bool transposed, double& dl,
                                                double& dd, double& du) {
  const int64_t q = (i / s) % m;
  const int64_t i0 = i - q * s, i1 = i0 + (m - 1) * s;
  dd = line_entry(rowptr, col, val, i, i);
  if (transposed) {
    dl = q > 0 ? line_entry(rowptr, col, val, i - s, i) : 0.0;
    du = q < m - 1 ? line_entry(rowptr, col, val, i + s, i) : 0.0;
  } else {
    dl = q > 0 ? line_entry(rowptr, col, val, i, i - s) : 0.0;
    du = q < m - 1 ? line_entry(rowptr, col, val, i, i + s) : 0.0;
  }
  if (q == 0) {
    const double gamma = 0.0 - dd;
    dd = dd - gamma;
  } else if (q == m - 1) {
    const double alpha = line_entry(rowptr, col, val, i0, i1), beta = line_entry(rowptr, col, val, i1, i0);
    const double gamma = 0.0 - line_entry(rowptr, col, val, i0, i0);
    dd = dd - alpha * beta / gamma;
  }
}
// rows of T from CSR(A): dl -> L.dl, diagonal -> L.ip, du -> L.w
// m > 0: the chain positions p = i / s form grid lines of m positions, and an entry that joins two
// lines (AMG_HIP_SM_LINE_ALT: +-nx across a plane end) stays out of T
// cyc (cyclic lines, m >= 3): 1 = T' of the Sherman-Morrison splitting (line_cyclic_row), 2 = its transpose
__host__ __device__ inline void line_extract_row(int64_t i, int64_t n, int64_t s, int64_t m, const int32_t* rowptr,
                                                 const int32_t* col, const double* val, double* dl, double* dd,
                                                 double* du, int cyc = 0) {
  if (cyc) {
    line_cyclic_row(i, s, m, rowptr, col, val, cyc == 2, dl[i], dd[i], du[i]);
    return;
  }
  double a = 0.0, b = 0.0, c = 0.0;
  const int64_t q = m > 0 ? (i / s) % m : 0;
  const bool lower = m <= 0 || q > 0, upper = m <= 0 || q < m - 1;
  for (int32_t p = rowptr[i]; p < rowptr[i + 1]; ++p) {
    const int64_t j = col[p];
    if (j == i) b = val[p];
    else if (j == i - s && lower) a = val[p];
    else if (j == i + s && upper) c = val[p];
  }
  dl[i] = a;
  dd[i] = b;
  du[i] = c;
}
// factor B_g of chain c in place; returns the first row with a bad pivot, or -1
__host__ __device__ inline int64_t line_factor_segment(const LineRef& L, int64_t g, int64_t c) {
  const int64_t n = L.n, s = L.s;
  const int64_t i0 = (g * LINE_SEG) * s + c;
  int64_t bad = -1;
  double cprev = 0.0, vprev = 0.0, wl = 0.0;
  int len = 0;
  for (int k = 0; k < LINE_INT; ++k) {
    const int64_t i = i0 + (int64_t)k * s;
    if (i >= n) break;
    const bool last = k == LINE_INT - 1 || i + s >= n;
    const double dl = L.dl[i], dd = L.ip[i], du = L.w[i];
    const double piv = k > 0 ? dd - dl * cprev : dd;
    if (bad < 0 && line_bad_pivot(piv)) bad = i;
    const double ip = 1.0 / piv;
    cprev = last ? 0.0 : du * ip;
    vprev = k > 0 ? (0.0 - dl * vprev) * ip : dl * ip;
    if (last) wl = du * ip;
    L.ip[i] = ip;
    L.cp[i] = cprev;
    L.v[i] = vprev;
    len = k + 1;
  }
  double vn = 0.0, wn = 0.0;
  for (int k = len - 1; k >= 0; --k) {
    const int64_t i = i0 + (int64_t)k * s;
    const double cp = L.cp[i];
    vn = L.v[i] - cp * vn;
    wn = k == len - 1 ? wl : 0.0 - cp * wn;
    L.v[i] = vn;
    L.w[i] = wn;
  }
  return bad;
}
// Schur complement on the separators of chain c and its factors; after line_factor_segment of all
__host__ __device__ inline int64_t line_factor_chain(const LineRef& L, int64_t c) {
  const int64_t n = L.n, s = L.s;
  int64_t bad = -1;
  double cprev = 0.0;
  for (int64_t g = 0;; ++g) {
    const int64_t i = (g * LINE_SEG + LINE_INT) * s + c;
    if (i >= n) break;
    const bool next = i + s < n;
    const double dl = L.dl[i], dd = L.ip[i], du = next ? L.w[i] : 0.0;
    const double vl = L.v[i - s], wl = L.w[i - s];
    const double vf = next ? L.v[i + s] : 0.0, wf = next ? L.w[i + s] : 0.0;
    const double lo = 0.0 - dl * vl;
    const double dg = (dd - dl * wl) - du * vf;
    const double up = 0.0 - du * wf;
    const double piv = g > 0 ? dg - lo * cprev : dg;
    if (bad < 0 && line_bad_pivot(piv)) bad = i;
    const double ip = 1.0 / piv;
    cprev = up * ip;
    L.v[i] = lo;
    L.ip[i] = ip;
    L.cp[i] = cprev;
  }
  return bad;
}
__host__ __device__ inline int64_t line_chains(int64_t n, int64_t s) { return s < n ? s : n; }
__host__ __device__ inline int64_t line_segments(int64_t n, int64_t s) {  // of the longest chain (chain 0)
  const int64_t m = (n + s - 1) / s;
  return (m + LINE_SEG - 1) / LINE_SEG;
}

__global__ __launch_bounds__(256) void line_extract_kernel(LineRef L, const int32_t* __restrict__ rowptr,
                                                           const int32_t* __restrict__ col,
                                                           const double* __restrict__ val) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < L.n) line_extract_row(i, L.n, L.s, L.m, rowptr, col, val, L.dl, L.ip, L.w, L.cyc);
}
__global__ __launch_bounds__(256) void line_factor_seg_kernel(LineRef L, int64_t nch, int64_t nseg,
                                                              unsigned long long* bad) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nch * nseg) return;
  const int64_t b = line_factor_segment(L, t / nch, t % nch);
  if (b >= 0) atomicMin(bad, (unsigned long long)b);
}
__global__ __launch_bounds__(256) void line_factor_chain_kernel(LineRef L, int64_t nch, unsigned long long* bad) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nch) return;
  const int64_t b = line_factor_chain(L, c);
  if (b >= 0) atomicMin(bad, (unsigned long long)b);
}

// The solve kernels are templates on the scalar type T and the panel pitch KP.  T: double for the
// cycle, float for the single-precision cycle (solver.cpp: "fp32 cycle"), which walks float copies of
// the same factors in the same order.  KP: r, y and u are row-major n x KP panels (entry (i, j) at
// i * KP + j, a 64-bit index; KP = 1: plain vectors, KP > 1: the panels of K-Block) and a lane works
// on one column j.  The factor arrays are indexed by row: the KP lanes of a row load the same factor
// words (served once) and one contiguous segment of every panel.  Per (row, column) the expressions
// and their order do not depend on KP, so column j of a panel has the bits of the plain vector.
// y_g = B_g^-1 r_g, lane = (segment, chain, column): the forward values stay in registers (the loops
// are fully unrolled), so the dependent chain is arithmetic only and the loads of r and of the
// factors run ahead of it
template <typename T, int KP>
__global__ __launch_bounds__(256) void line_seg_kernel(int64_t n, int64_t s, int64_t nch, int64_t nseg,
                                                       const T* __restrict__ r, const T* __restrict__ dl,
                                                       const T* __restrict__ ip, const T* __restrict__ cp,
                                                       T* __restrict__ y) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nch * nseg * KP) return;
  const int j = (int)(t % KP);
  const int64_t q = t / KP;
  const int64_t g = q / nch, c = q - g * nch;
  const int64_t i0 = (g * LINE_SEG) * s + c;
  T yv[LINE_INT];
  T prev = T(0);
#pragma unroll
  for (int k = 0; k < LINE_INT; ++k) {
    const int64_t i = i0 + (int64_t)k * s;
    if (i < n) prev = k > 0 ? (r[i * KP + j] - dl[i] * prev) * ip[i] : r[i * KP + j] * ip[i];
    else prev = T(0);
    yv[k] = prev;
  }
  T nxt = T(0);
#pragma unroll
  for (int k = LINE_INT - 1; k >= 0; --k) {
    const int64_t i = i0 + (int64_t)k * s;
    if (i < n) {
      nxt = yv[k] - cp[i] * nxt;
      y[i * KP + j] = nxt;
    }
  }
}

// right-hand side of the reduced system at separator row i, column j
template <typename T, int KP>
__device__ inline T line_sep_rhs(int64_t i, int j, int64_t n, int64_t s, const T* r, const T* dl, const T* w,
                                 const T* y) {
  T b = r[i * KP + j] - dl[i] * y[(i - s) * KP + j];
  if (i + s < n) b = b - w[i] * y[(i + s) * KP + j];
  return b;
}
// many chains: lane = (chain, column), neighbouring lanes neighbouring addresses.  Each batch of
// LINE_BATCH separators is loaded before its dependent steps run, so a chain of m / 32 separators
// costs m / (32 LINE_BATCH) memory latencies per direction, once for the KP columns.
constexpr int LINE_BATCH = 8;
template <typename T, int KP>
__global__ __launch_bounds__(64) void line_sep_many_kernel(int64_t n, int64_t s, int64_t nch, const T* r,
                                                           const T* dl, const T* ip, const T* cp, const T* v,
                                                           const T* w, T* y) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nch * KP) return;
  const int j = (int)(t % KP);
  const int64_t c = t / KP;
  const int64_t step = (int64_t)LINE_SEG * s;
  const int64_t first = (int64_t)LINE_INT * s + c;
  if (first >= n) return;
  const int64_t nsep = (n - 1 - first) / step + 1;
  T tv = T(0);
  for (int64_t g0 = 0; g0 < nsep; g0 += LINE_BATCH) {
    T b[LINE_BATCH], lo[LINE_BATCH], pv[LINE_BATCH];
#pragma unroll
    for (int k = 0; k < LINE_BATCH; ++k) {
      const int64_t i = first + (g0 + k) * step;
      const bool on = g0 + k < nsep;
      b[k] = on ? line_sep_rhs<T, KP>(i, j, n, s, r, dl, w, y) : T(0);
      lo[k] = on ? v[i] : T(0);
      pv[k] = on ? ip[i] : T(0);
    }
#pragma unroll
    for (int k = 0; k < LINE_BATCH; ++k) {
      if (g0 + k < nsep) {
        tv = (b[k] - lo[k] * tv) * pv[k];
        y[(first + (g0 + k) * step) * KP + j] = tv;
      }
    }
  }
  T x = T(0);
  for (int64_t g1 = nsep; g1 > 0; g1 -= LINE_BATCH) {  // separators g1-1, g1-2, ...
    T tt[LINE_BATCH], cc[LINE_BATCH];
#pragma unroll
    for (int k = 0; k < LINE_BATCH; ++k) {
      const int64_t g = g1 - 1 - k;
      const int64_t i = first + g * step;
      tt[k] = g >= 0 ? y[i * KP + j] : T(0);
      cc[k] = g >= 0 ? cp[i] : T(0);
    }
#pragma unroll
    for (int k = 0; k < LINE_BATCH; ++k) {
      const int64_t g = g1 - 1 - k;
      if (g >= 0) {
        x = tt[k] - cc[k] * x;
        y[(first + g * step) * KP + j] = x;
      }
    }
  }
}
// few long chains: one workgroup per chain.  All lanes stage a chunk of the reduced system in LDS
// (lo and pv once, b per column), lanes 0 .. KP - 1 each walk one column there (an LDS round trip
// per step instead of a memory one) and keep the recurrence in a register from chunk to chunk, all
// lanes write the chunk back.  Same arithmetic in the same order as line_sep_many_kernel.
// Chunks of line_few_chunk_c(KP) separators, (KP + 2) T of LDS each: 24 KB in double and 12 KB in
// float up to KP = 4, 36 KB in double at KP = 16.
constexpr int LINE_FEW_CHUNK = 1024;
__host__ __device__ constexpr int line_few_chunk_c(int kp) { return kp <= 4 ? LINE_FEW_CHUNK : 4 * LINE_FEW_CHUNK / kp; }
template <typename T, int KP>
__global__ __launch_bounds__(256) void line_sep_few_kernel(int64_t n, int64_t s, const T* r, const T* dl,
                                                           const T* ip, const T* cp, const T* v, const T* w,
                                                           T* y) {
  constexpr int CH = line_few_chunk_c(KP);
  __shared__ T b[CH * KP], lo[CH], pv[CH];
  const int tid = threadIdx.x;
  const int64_t c = blockIdx.x;
  const int64_t step = (int64_t)LINE_SEG * s;
  const int64_t first = (int64_t)LINE_INT * s + c;
  if (first >= n) return;  // the whole workgroup
  const int64_t nsep = (n - 1 - first) / step + 1;
  T carry = T(0);  // lanes < KP: the recurrence of column tid
  for (int64_t g0 = 0; g0 < nsep; g0 += CH) {
    const int m = (int)(nsep - g0 < CH ? nsep - g0 : CH);
    for (int e = tid; e < m * KP; e += 256) {
      const int g = e / KP, j = e % KP;
      const int64_t i = first + (g0 + g) * step;
      b[e] = line_sep_rhs<T, KP>(i, j, n, s, r, dl, w, y);
      if (j == 0) {
        lo[g] = v[i];
        pv[g] = ip[i];
      }
    }
    __syncthreads();
    if (tid < KP) {
      T t = carry;
      for (int g = 0; g < m; ++g) {
        t = (b[g * KP + tid] - lo[g] * t) * pv[g];
        b[g * KP + tid] = t;
      }
      carry = t;
    }
    __syncthreads();
    for (int e = tid; e < m * KP; e += 256) y[(first + (g0 + e / KP) * step) * KP + e % KP] = b[e];
    __syncthreads();
  }
  carry = T(0);
  for (int64_t g1 = nsep; g1 > 0; g1 -= CH) {  // separators [g1 - m, g1)
    const int m = (int)(g1 < CH ? g1 : CH);
    const int64_t gb = g1 - m;
    for (int e = tid; e < m * KP; e += 256) {
      const int g = e / KP, j = e % KP;
      const int64_t i = first + (gb + g) * step;
      b[e] = y[i * KP + j];
      if (j == 0) lo[g] = cp[i];
    }
    __syncthreads();
    if (tid < KP) {
      T x = carry;
      for (int g = m - 1; g >= 0; --g) {
        x = b[g * KP + tid] - lo[g] * x;
        b[g * KP + tid] = x;
      }
      carry = x;
    }
    __syncthreads();
    for (int e = tid; e < m * KP; e += 256) y[(first + (gb + e / KP) * step) * KP + e % KP] = b[e];
    __syncthreads();
  }
}

// x_i = y_i - v_i x_(separator before) - w_i x_(separator after); u_i += omega x_i, lane = (row, column)
template <typename T, int KP>
__global__ __launch_bounds__(256) void line_update_kernel(int64_t n, uint32_t s, const T* __restrict__ y,
                                                          const T* __restrict__ v, const T* __restrict__ w,
                                                          T omega, T* __restrict__ u) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * KP) return;
  const int64_t i = e / KP;  // < 2^31: the row, not the panel index, goes through the 32-bit division
  const int j = (int)(e % KP);
  const uint32_t p = (uint32_t)i / s;
  const uint32_t k = p % LINE_SEG;
  T x = y[e];
  if (k != LINE_INT) {
    const int64_t before = i - ((int64_t)k + 1) * s;
    const int64_t after = i + (int64_t)(LINE_INT - k) * s;
    if (before >= 0) x = x - v[i] * y[before * KP + j];
    if (after < n) x = x - w[i] * y[after * KP + j];
  }
  u[e] = u[e] + omega * x;
}

// ---- stride rule: w(d) = sum of |a_ij| over |j - i| = d >= 1 -----------------------------------
// Level matrices have a handful of distinct distances, so every workgroup first sums into a small
// LDS table keyed by distance and flushes one atomic per used slot; a full table falls through to
// the global atomic.
constexpr int LINE_DSLOTS = 32;
__global__ __launch_bounds__(256) void line_dist_kernel(int64_t n, const int32_t* __restrict__ rowptr,
                                                        const int32_t* __restrict__ col,
                                                        const double* __restrict__ val, double* wd) {
  __shared__ int key[LINE_DSLOTS];
  __shared__ double sum[LINE_DSLOTS];
  if (threadIdx.x < LINE_DSLOTS) {
    key[threadIdx.x] = 0;
    sum[threadIdx.x] = 0.0;
  }
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    for (int32_t p = rowptr[i]; p < rowptr[i + 1]; ++p) {
      const int64_t dj = (int64_t)col[p] - i;
      const int d = (int)(dj < 0 ? -dj : dj);
      if (d == 0) continue;
      const double a = fabs(val[p]);
      int slot = d % LINE_DSLOTS;
      bool done = false;
      for (int probe = 0; probe < LINE_DSLOTS && !done; ++probe) {
        const int old = atomicCAS(&key[slot], 0, d);
        if (old == 0 || old == d) {
          atomicAdd(&sum[slot], a);
          done = true;
        }
        slot = (slot + 1) % LINE_DSLOTS;
      }
      if (!done) atomicAdd(&wd[d], a);
    }
  }
  __syncthreads();
  if (threadIdx.x < LINE_DSLOTS && key[threadIdx.x] != 0) atomicAdd(&wd[key[threadIdx.x]], sum[threadIdx.x]);
}
// out[0] = bits of max_d w(d) (non-negative doubles order like their bit patterns)
__global__ __launch_bounds__(256) void line_wmax_kernel(int64_t n, const double* __restrict__ wd,
                                                        unsigned long long* out) {
  const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x + 1;
  if (d < n && wd[d] > 0.0) atomicMax(&out[0], (unsigned long long)__double_as_longlong(wd[d]));
}
// out[1] = the largest d with w(d) >= (1 - 1e-9) max w
__global__ __launch_bounds__(256) void line_pick_kernel(int64_t n, const double* __restrict__ wd,
                                                        unsigned long long* out) {
  const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x + 1;
  if (d >= n) return;
  const double mx = __longlong_as_double((long long)out[0]);
  if (mx > 0.0 && wd[d] >= (1.0 - 1e-9) * mx) atomicMax(&out[1], (unsigned long long)d);
}
__global__ void line_init2_kernel(unsigned long long* out, unsigned long long a, unsigned long long b) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    out[0] = a;
    out[1] = b;
  }
}
inline dim3 line_grid(int64_t threads, int block = 256) { return dim3((unsigned)((threads + block - 1) / block)); }
}  // namespace

hipError_t launch_line_stride(int64_t n, const int32_t* rowptr, const int32_t* col, const double* val, double* wd,
                              uint64_t* out, hipStream_t st) {
  auto* o = reinterpret_cast<unsigned long long*>(out);
  hipLaunchKernelGGL(line_init2_kernel, dim3(1), dim3(64), 0, st, o, 0ull, 1ull);
  hipError_t e = hipMemsetAsync(wd, 0, sizeof(double) * (size_t)n, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(line_dist_kernel, line_grid(n), dim3(256), 0, st, n, rowptr, col, val, wd);
  if (n > 1) {
    hipLaunchKernelGGL(line_wmax_kernel, line_grid(n - 1), dim3(256), 0, st, n, wd, o);
    hipLaunchKernelGGL(line_pick_kernel, line_grid(n - 1), dim3(256), 0, st, n, wd, o);
  }
  return hipGetLastError();
}
int64_t line_stride_host(int64_t n, const int32_t* rowptr, const int32_t* col, const double* val) {
  std::vector<double> wd((size_t)n, 0.0);
  for (int64_t i = 0; i < n; ++i)
    for (int32_t p = rowptr[i]; p < rowptr[i + 1]; ++p) {
      const int64_t d = col[p] < i ? i - col[p] : col[p] - i;
      if (d > 0) wd[(size_t)d] += std::fabs(val[p]);
    }
  double mx = 0.0;
  for (int64_t d = 1; d < n; ++d) mx = std::max(mx, wd[(size_t)d]);
  int64_t s = 1;
  if (mx > 0.0)
    for (int64_t d = 1; d < n; ++d)
      if (wd[(size_t)d] >= (1.0 - 1e-9) * mx) s = d;
  return s;
}

hipError_t launch_line_setup(const LineRef& L, const int32_t* rowptr, const int32_t* col, const double* val,
                             uint64_t* bad, hipStream_t st) {
  // s <= n < 2^31 bounds every index product of the kernels (at most 64 s + n) well inside int64
  if (L.n <= 0 || L.s < 1 || L.s > L.n || L.n >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
  auto* o = reinterpret_cast<unsigned long long*>(bad);
  const int64_t nch = line_chains(L.n, L.s), nseg = line_segments(L.n, L.s);
  hipLaunchKernelGGL(line_init2_kernel, dim3(1), dim3(64), 0, st, o, ~0ull, 0ull);
  hipLaunchKernelGGL(line_extract_kernel, line_grid(L.n), dim3(256), 0, st, L, rowptr, col, val);
  hipLaunchKernelGGL(line_factor_seg_kernel, line_grid(nch * nseg), dim3(256), 0, st, L, nch, nseg, o);
  hipLaunchKernelGGL(line_factor_chain_kernel, line_grid(nch), dim3(256), 0, st, L, nch, o);
  return hipGetLastError();
}
int64_t line_setup_host(int64_t n, int64_t s, const int32_t* rowptr, const int32_t* col, const double* val,
                        int64_t m, int cyc) {
  std::vector<double> a[5];
  for (auto& x : a) x.assign((size_t)n, 0.0);
  LineRef L;
  L.n = n;
  L.s = s < n ? s : n;  // every stride >= n: each row its own chain
  L.dl = a[0].data();
  L.ip = a[1].data();
  L.cp = a[2].data();
  L.v = a[3].data();
  L.w = a[4].data();
  for (int64_t i = 0; i < n; ++i) line_extract_row(i, n, s, m, rowptr, col, val, L.dl, L.ip, L.w, cyc);
  const int64_t nch = line_chains(n, L.s), nseg = line_segments(n, L.s);
  int64_t bad = -1;
  auto note = [&](int64_t b) {
    if (b >= 0 && (bad < 0 || b < bad)) bad = b;
  };
  for (int64_t g = 0; g < nseg; ++g)
    for (int64_t c = 0; c < nch; ++c) note(line_factor_segment(L, g, c));
  for (int64_t c = 0; c < nch; ++c) note(line_factor_chain(L, c));
  return bad;
}

bool line_few_chains(int64_t s) { return s < 64; }
int block_line_few_chunk(int kp) { return line_few_chunk_c(kp); }
namespace {
inline bool block_kp_ok(int kp) { return kp == 1 || kp == 2 || kp == 4 || kp == 8 || kp == 16; }
// CALL(KP) with the pitch as a constant
#define AMG_BLOCK_KP(kp, CALL) \
  switch (kp) {                \
    case 1: CALL(1); break;    \
    case 2: CALL(2); break;    \
    case 4: CALL(4); break;    \
    case 8: CALL(8); break;    \
    default: CALL(16); break;  \
  }
template <typename T, int KP>
hipError_t line_solve_t(const LineRefT<T>& L, const T* r, T* y, T* u, T omega, hipStream_t st) {
  const int64_t n = L.n, s = L.s;
  if (n <= 0 || s < 1 || s > n || n >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
  const int64_t nch = line_chains(n, s), nseg = line_segments(n, s);
  hipLaunchKernelGGL((line_seg_kernel<T, KP>), line_grid(nch * nseg * KP), dim3(256), 0, st, n, s, nch, nseg, r,
                     (const T*)L.dl, (const T*)L.ip, (const T*)L.cp, y);
  if ((int64_t)LINE_INT * s < n) {  // the level has separators
    if (line_few_chains(s)) {
      hipLaunchKernelGGL((line_sep_few_kernel<T, KP>), dim3((unsigned)nch), dim3(256), 0, st, n, s, r, (const T*)L.dl,
                         (const T*)L.ip, (const T*)L.cp, (const T*)L.v, (const T*)L.w, y);
    } else {
      hipLaunchKernelGGL((line_sep_many_kernel<T, KP>), line_grid(nch * KP, 64), dim3(64), 0, st, n, s, nch, r,
                         (const T*)L.dl, (const T*)L.ip, (const T*)L.cp, (const T*)L.v, (const T*)L.w, y);
    }
  }
  hipLaunchKernelGGL((line_update_kernel<T, KP>), line_grid(n * KP), dim3(256), 0, st, n, (uint32_t)s, (const T*)y,
                     (const T*)L.v, (const T*)L.w, omega, u);
  return hipGetLastError();
}
}  // namespace
hipError_t launch_line_solve(const LineRef& L, const double* r, double* y, double* u, double omega,
                             hipStream_t st) {
  return line_solve_t<double, 1>(L, r, y, u, omega, st);
}
hipError_t launch_line_solve_f32(const LineRefT<float>& L, const float* r, float* y, float* u, float omega,
                                 hipStream_t st) {
  return line_solve_t<float, 1>(L, r, y, u, omega, st);
}
hipError_t launch_block_line_solve(int kp, const LineRef& L, const double* r, double* y, double* u, double omega,
                                   hipStream_t st) {
  if (!block_kp_ok(kp)) return hipErrorInvalidValue;
  hipError_t e = hipSuccess;
#define LINE_KP(KP) e = line_solve_t<double, KP>(L, r, y, u, omega, st)
  AMG_BLOCK_KP(kp, LINE_KP)
#undef LINE_KP
  return e;
}

// ---- K-LineX: the x lines of a tensor grid (AMG_HIP_SM_LINE_ALT; kernels.hpp: LineXRef) --------
// T_x is tridiagonal on the flat index with its couplings across line ends removed, so the plain
// Thomas factors (dl, ip = 1 / pivot, cp = upper / pivot) carry dl = 0 on the first and cp = 0 on
// the last row of every line: a walk along the flat index restarts by itself at every line.  The
// level is cut into runs of `len` rows (whole lines: one line of nx >= LINEX_COLS rows, or
// LINEX_COLS / nx short ones).  One wave owns LINEX_RUNS neighbouring runs and walks them in
// chunks of LINEX_COLS columns: all 64 lanes load the chunk (a 512-byte row of every run:
// neighbouring lanes, neighbouring addresses) into LDS, lanes 0 .. LINEX_RUNS - 1 each walk one
// run's row of the chunk there and carry the recurrence in a register to the next chunk, all lanes
// write the chunk back.  The loads of the next chunk are issued before the walk of this one.
//   linex_kernel<LX_FACTOR>  dd, du -> ip, cp (setup)
//   linex_kernel<LX_FWD>     r <- y: y_i = (r_i - dl_i y_(i-1)) ip_i          (in place)
//   linex_kernel<LX_BWD>     x_i = y_i - cp_i x_(i+1); u_i += omega x_i       (chunks descending)
namespace {
enum { LX_FACTOR = 0, LX_FWD = 1, LX_BWD = 2 };
constexpr int LINEX_PITCH = LINEX_COLS + 1;  // doubles per LDS row: the walking lanes hit different banks

__host__ __device__ inline void linex_row(int64_t i, int64_t nx, const int32_t* rowptr, const int32_t* col,
                                          const double* val, double& dl, double& dd, double& du, int cyc = 0) {
  if (cyc) {  // cyclic x lines: T' or its transpose (K-Line: line_cyclic_row)
    line_cyclic_row(i, 1, nx, rowptr, col, val, cyc == 2, dl, dd, du);
    return;
  }
  const int64_t x = i % nx;
  dl = dd = du = 0.0;
  for (int32_t p = rowptr[i]; p < rowptr[i + 1]; ++p) {
    const int64_t j = col[p];
    if (j == i) dd = val[p];
    else if (j == i - 1 && x > 0) dl = val[p];
    else if (j == i + 1 && x < nx - 1) du = val[p];
  }
}
__global__ __launch_bounds__(256) void linex_extract_kernel(LineXRef L, const int32_t* __restrict__ rowptr,
                                                            const int32_t* __restrict__ col,
                                                            const double* __restrict__ val) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < L.n) linex_row(i, L.nx, rowptr, col, val, L.dl[i], L.ip[i], L.cp[i], L.cyc);
}

// a, b, c: the three arrays a chunk reads (FACTOR: dl, dd, du; FWD: r, dl, ip; BWD: y, cp, u);
// o1, o2: what it writes (FACTOR: ip, cp; FWD: y = a; BWD: u = c)
// T = float (FWD and BWD only): the same chunks of LINEX_COLS columns, 256 B per row and array
template <int MODE, typename T>
__global__ __launch_bounds__(64) void linex_kernel(int64_t n, int64_t len, int64_t nruns, const T* a, const T* b,
                                                   const T* c, T* o1, T* o2, T omega, unsigned long long* bad) {
  __shared__ T sa[LINEX_RUNS * LINEX_PITCH], sb[LINEX_RUNS * LINEX_PITCH], sc[LINEX_RUNS * LINEX_PITCH];
  const int lane = threadIdx.x;
  const int64_t run0 = (int64_t)blockIdx.x * LINEX_RUNS;
  const int64_t nchunks = (len + LINEX_COLS - 1) / LINEX_COLS;
  T ra[LINEX_RUNS], rb[LINEX_RUNS], rc[LINEX_RUNS];
  // row of run q at this lane's column of chunk ch, or -1 outside the run / the level
  auto row_of = [&](int q, int64_t ch) -> int64_t {
    const int64_t run = run0 + q, k = ch * LINEX_COLS + lane;
    if (run >= nruns || k >= len) return -1;
    const int64_t i = run * len + k;
    return i < n ? i : -1;
  };
  auto fetch = [&](int64_t ch) {
#pragma unroll
    for (int q = 0; q < LINEX_RUNS; ++q) {
      const int64_t i = row_of(q, ch);
      ra[q] = i >= 0 ? a[i] : T(0);
      rb[q] = i >= 0 ? b[i] : T(0);
      rc[q] = i >= 0 ? c[i] : T(0);
    }
  };
  T carry = T(0);  // lanes < LINEX_RUNS: cp (FACTOR), y (FWD) or x (BWD) of the row walked last
  fetch(MODE == LX_BWD ? nchunks - 1 : 0);
  for (int64_t t = 0; t < nchunks; ++t) {
    const int64_t ch = MODE == LX_BWD ? nchunks - 1 - t : t;
#pragma unroll
    for (int q = 0; q < LINEX_RUNS; ++q) {
      sa[q * LINEX_PITCH + lane] = ra[q];
      sb[q * LINEX_PITCH + lane] = rb[q];
      sc[q * LINEX_PITCH + lane] = rc[q];
    }
    __syncthreads();
    if (t + 1 < nchunks) fetch(MODE == LX_BWD ? ch - 1 : ch + 1);
    if (lane < LINEX_RUNS) {
      T* pa = sa + lane * LINEX_PITCH;
      T* pb = sb + lane * LINEX_PITCH;
      T* pc = sc + lane * LINEX_PITCH;
      if (MODE == LX_FACTOR) {
        const int64_t i0 = (run0 + lane) * len + ch * LINEX_COLS;
        int64_t first_bad = -1;
#pragma unroll 8
        for (int k = 0; k < LINEX_COLS; ++k) {
          const T piv = pb[k] - pa[k] * carry;
          const bool in = run0 + lane < nruns && ch * LINEX_COLS + k < len && i0 + k < n;
          if (in && first_bad < 0 && line_bad_pivot(piv)) first_bad = i0 + k;
          const T ip = in ? T(1) / piv : T(0);
          carry = pc[k] * ip;
          pb[k] = ip;
          pc[k] = carry;
        }
        if (first_bad >= 0) atomicMin(bad, (unsigned long long)first_bad);
      } else if (MODE == LX_FWD) {
#pragma unroll 8
        for (int k = 0; k < LINEX_COLS; ++k) {
          carry = (pa[k] - pb[k] * carry) * pc[k];
          pa[k] = carry;
        }
      } else {
#pragma unroll 8
        for (int k = LINEX_COLS - 1; k >= 0; --k) {
          carry = pa[k] - pb[k] * carry;
          pa[k] = carry;
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < LINEX_RUNS; ++q) {
      const int64_t i = row_of(q, ch);
      if (i < 0) continue;
      if (MODE == LX_FACTOR) {
        o1[i] = sb[q * LINEX_PITCH + lane];
        o2[i] = sc[q * LINEX_PITCH + lane];
      } else if (MODE == LX_FWD) {
        o1[i] = sa[q * LINEX_PITCH + lane];
      } else {
        o1[i] = sc[q * LINEX_PITCH + lane] + omega * sa[q * LINEX_PITCH + lane];
      }
    }
    __syncthreads();
  }
}
template <typename T>
inline bool linex_ok(const LineXRefT<T>& L) {
  return L.n > 0 && L.nx >= 1 && L.n < ((int64_t)1 << 31) && L.n % L.nx == 0;
}
}  // namespace

int64_t linex_run(int64_t nx) { return nx >= LINEX_COLS ? nx : nx * (LINEX_COLS / nx); }

hipError_t launch_linex_setup(const LineXRef& L, const int32_t* rowptr, const int32_t* col, const double* val,
                              uint64_t* bad, hipStream_t st) {
  if (!linex_ok(L)) return hipErrorInvalidValue;
  auto* o = reinterpret_cast<unsigned long long*>(bad);
  const int64_t len = linex_run(L.nx), nruns = (L.n + len - 1) / len;
  hipLaunchKernelGGL(line_init2_kernel, dim3(1), dim3(64), 0, st, o, ~0ull, 0ull);
  hipLaunchKernelGGL(linex_extract_kernel, line_grid(L.n), dim3(256), 0, st, L, rowptr, col, val);
  hipLaunchKernelGGL((linex_kernel<LX_FACTOR, double>), line_grid(nruns, LINEX_RUNS), dim3(64), 0, st, L.n, len, nruns, L.dl,
                     L.ip, L.cp, L.ip, L.cp, 0.0, o);
  return hipGetLastError();
}
int64_t linex_setup_host(int64_t n, int64_t nx, const int32_t* rowptr, const int32_t* col, const double* val,
                         int cyc) {
  double cprev = 0.0;
  for (int64_t i = 0; i < n; ++i) {
    double dl, dd, du;
    linex_row(i, nx, rowptr, col, val, dl, dd, du, cyc);
    const double piv = dd - dl * cprev;
    if (line_bad_pivot(piv)) return i;
    cprev = du * (1.0 / piv);
  }
  return -1;
}
namespace {
template <typename T>
hipError_t linex_solve_t(const LineXRefT<T>& L, T* r, T* u, T omega, hipStream_t st) {
  if (!linex_ok(L)) return hipErrorInvalidValue;
  const int64_t n = L.n, len = linex_run(L.nx), nruns = (n + len - 1) / len;
  const dim3 grid = line_grid(nruns, LINEX_RUNS);
  hipLaunchKernelGGL((linex_kernel<LX_FWD, T>), grid, dim3(64), 0, st, n, len, nruns, (const T*)r, (const T*)L.dl,
                     (const T*)L.ip, r, (T*)nullptr, T(0), (unsigned long long*)nullptr);
  hipLaunchKernelGGL((linex_kernel<LX_BWD, T>), grid, dim3(64), 0, st, n, len, nruns, (const T*)r, (const T*)L.cp,
                     (const T*)u, u, (T*)nullptr, omega, (unsigned long long*)nullptr);
  return hipGetLastError();
}
}  // namespace
hipError_t launch_linex_solve(const LineXRef& L, double* r, double* u, double omega, hipStream_t st) {
  return linex_solve_t(L, r, u, omega, st);
}
hipError_t launch_linex_solve_f32(const LineXRefT<float>& L, float* r, float* u, float omega, hipStream_t st) {
  return linex_solve_t(L, r, u, omega, st);
}

// ---- K-LineSeam: the rank-one correction of a cyclic line solve (kernels.hpp: SeamRef) ----------
// Per line: fac = (sum over the line of p_i r_i) / den; r(i0) -= fac gamma; r(i1) -= fac beta.  The
// open solve with the factors of T' that follows then gives T_a^-1 r of the cyclic T_a.
//   seamx_kernel<W>     x lines (s = 1).  W = 4 .. 64 lanes run across a line, 64 / W lines to a wave.
//                       A lane sums its columns k, k + W, k + 2 W, ... in ascending order (the loads of
//                       SEAM_BATCH columns are issued before the first is used), a butterfly of log2 W
//                       __shfl_xor steps adds the lanes, lane 0 of the line corrects the two ends.
//   seam_stride_kernel  y and z lines.  One lane per line walks its m rows at stride s in ascending
//                       order; neighbouring lanes hold neighbouring lines, so every step is a
//                       coalesced row of loads.
// The order of every sum is fixed by (m, s) alone.
namespace {
constexpr int SEAM_BATCH = 4;
template <int W, typename T>
__global__ __launch_bounds__(256) void seamx_kernel(int64_t nlines, int64_t m, const T* __restrict__ p,
                                                    const T* __restrict__ coef, T* r) {
  constexpr int LPW = 64 / W;  // lines per wave
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
  const int k = lane & (W - 1);
  const int64_t line = wave * LPW + lane / W;
  const bool live = line < nlines;
  const int64_t i0 = live ? line * m : 0;
  T acc = T(0);
  if (live) {
    for (int64_t c0 = k; c0 < m; c0 += (int64_t)SEAM_BATCH * W) {
      T pv[SEAM_BATCH], rv[SEAM_BATCH];
#pragma unroll
      for (int j = 0; j < SEAM_BATCH; ++j) {
        const int64_t c = c0 + (int64_t)j * W;
        pv[j] = c < m ? p[i0 + c] : T(0);
        rv[j] = c < m ? r[i0 + c] : T(0);
      }
#pragma unroll
      for (int j = 0; j < SEAM_BATCH; ++j)
        if (c0 + (int64_t)j * W < m) acc = acc + pv[j] * rv[j];
    }
  }
#pragma unroll
  for (int off = W / 2; off >= 1; off >>= 1) acc = acc + __shfl_xor(acc, off, W);
  if (live && k == 0) {
    const T fac = acc / coef[line];
    const int64_t i1 = i0 + m - 1;
    r[i0] = r[i0] - fac * coef[nlines + line];
    r[i1] = r[i1] - fac * coef[2 * nlines + line];
  }
}
constexpr int SEAM_WALK = 8;
// r: an n x KP panel as in K-Line, lane = (line, column)
template <typename T, int KP>
__global__ __launch_bounds__(256) void seam_stride_kernel(int64_t nlines, int64_t s, int64_t m,
                                                          const T* __restrict__ p, const T* __restrict__ coef,
                                                          T* r) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t line = t / KP;
  const int j = (int)(t % KP);
  if (line >= nlines) return;
  const int64_t b = line / s;
  const int64_t i0 = b * s * m + (line - b * s);
  T acc = T(0);
  for (int64_t k0 = 0; k0 < m; k0 += SEAM_WALK) {
    T pv[SEAM_WALK], rv[SEAM_WALK];
#pragma unroll
    for (int q = 0; q < SEAM_WALK; ++q) {
      const bool on = k0 + q < m;
      pv[q] = on ? p[i0 + (k0 + q) * s] : T(0);
      rv[q] = on ? r[(i0 + (k0 + q) * s) * KP + j] : T(0);
    }
#pragma unroll
    for (int q = 0; q < SEAM_WALK; ++q)
      if (k0 + q < m) acc = acc + pv[q] * rv[q];
  }
  const T fac = acc / coef[line];
  const int64_t e0 = i0 * KP + j, e1 = (i0 + (m - 1) * s) * KP + j;
  r[e0] = r[e0] - fac * coef[nlines + line];
  r[e1] = r[e1] - fac * coef[2 * nlines + line];
}

// set-up: the two right-hand sides u = gamma e(i0) + beta e(i1), v = e(i0) + (alpha / gamma) e(i1)
__host__ __device__ inline void seam_wrap(int64_t i0, int64_t s, int64_t m, const int32_t* rowptr, const int32_t* col,
                                          const double* val, double& alpha, double& beta, double& gamma) {
  const int64_t i1 = i0 + (m - 1) * s;
  alpha = line_entry(rowptr, col, val, i0, i1);
  beta = line_entry(rowptr, col, val, i1, i0);
  gamma = 0.0 - line_entry(rowptr, col, val, i0, i0);
}
__global__ __launch_bounds__(256) void seam_rhs_kernel(int64_t n, int64_t s, int64_t m,
                                                       const int32_t* __restrict__ rowptr,
                                                       const int32_t* __restrict__ col,
                                                       const double* __restrict__ val, double* u, double* v) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t q = (i / s) % m;
  double uu = 0.0, vv = 0.0;
  if (q == 0 || q == m - 1) {
    double alpha, beta, gamma;
    seam_wrap(i - q * s, s, m, rowptr, col, val, alpha, beta, gamma);
    uu = q == 0 ? gamma : beta;
    vv = q == 0 ? 1.0 : alpha / gamma;
  }
  u[i] = uu;
  v[i] = vv;
}
__host__ __device__ inline double seam_den(double alpha, double gamma, double q0, double q1) {
  return (1.0 + q0) + (alpha / gamma) * q1;
}
// coef = den | gamma | beta of every line from q = T'^-1 u; bad[0] = first row of the first line whose
// den is zero or not finite
__global__ __launch_bounds__(256) void seam_coef_kernel(int64_t nlines, int64_t s, int64_t m,
                                                        const int32_t* __restrict__ rowptr,
                                                        const int32_t* __restrict__ col,
                                                        const double* __restrict__ val,
                                                        const double* __restrict__ q, double* coef,
                                                        unsigned long long* bad) {
  const int64_t line = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (line >= nlines) return;
  const int64_t b = line / s;
  const int64_t i0 = b * s * m + (line - b * s), i1 = i0 + (m - 1) * s;
  double alpha, beta, gamma;
  seam_wrap(i0, s, m, rowptr, col, val, alpha, beta, gamma);
  const double den = seam_den(alpha, gamma, q[i0], q[i1]);
  coef[line] = den;
  coef[nlines + line] = gamma;
  coef[2 * nlines + line] = beta;
  if (line_bad_pivot(den)) atomicMin(bad, (unsigned long long)i0);
}
inline bool seam_ok(int64_t n, int64_t s, int64_t m) {
  return n > 0 && n < ((int64_t)1 << 31) && s >= 1 && m >= 3 && s * m <= n && n % (s * m) == 0;
}
}  // namespace

hipError_t launch_seam_rhs(int64_t n, int64_t s, int64_t m, const int32_t* rowptr, const int32_t* col,
                           const double* val, double* u, double* v, hipStream_t st) {
  if (!seam_ok(n, s, m)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(seam_rhs_kernel, line_grid(n), dim3(256), 0, st, n, s, m, rowptr, col, val, u, v);
  return hipGetLastError();
}
hipError_t launch_seam_coef(int64_t n, int64_t s, int64_t m, const int32_t* rowptr, const int32_t* col,
                            const double* val, const double* q, double* coef, uint64_t* bad, hipStream_t st) {
  if (!seam_ok(n, s, m)) return hipErrorInvalidValue;
  auto* o = reinterpret_cast<unsigned long long*>(bad);
  hipLaunchKernelGGL(line_init2_kernel, dim3(1), dim3(64), 0, st, o, ~0ull, 0ull);
  hipLaunchKernelGGL(seam_coef_kernel, line_grid(n / m), dim3(256), 0, st, n / m, s, m, rowptr, col, val, q, coef, o);
  return hipGetLastError();
}
int64_t seam_setup_host(int64_t n, int64_t s, int64_t m, const int32_t* rowptr, const int32_t* col,
                        const double* val) {
  std::vector<double> cp((size_t)m), y((size_t)m);
  for (int64_t line = 0; line < n / m; ++line) {
    const int64_t b = line / s;
    const int64_t i0 = b * s * m + (line - b * s);
    double alpha, beta, gamma;
    seam_wrap(i0, s, m, rowptr, col, val, alpha, beta, gamma);
    double cprev = 0.0, yprev = 0.0;  // plain Thomas on T' q = gamma e(i0) + beta e(i1)
    for (int64_t k = 0; k < m; ++k) {
      double dl, dd, du;
      line_cyclic_row(i0 + k * s, s, m, rowptr, col, val, false, dl, dd, du);
      const double ip = 1.0 / (dd - dl * cprev);
      const double rhs = k == 0 ? gamma : k == m - 1 ? beta : 0.0;
      yprev = (rhs - dl * yprev) * ip;
      cprev = du * ip;
      y[(size_t)k] = yprev;
      cp[(size_t)k] = cprev;
    }
    double x = 0.0, q0 = 0.0, q1 = 0.0;
    for (int64_t k = m - 1; k >= 0; --k) {
      x = y[(size_t)k] - cp[(size_t)k] * x;
      if (k == m - 1) q1 = x;
      if (k == 0) q0 = x;
    }
    if (line_bad_pivot(seam_den(alpha, gamma, q0, q1))) return i0;
  }
  return -1;
}
namespace {
template <typename T>
hipError_t line_seam_t(const SeamRefT<T>& S, T* r, hipStream_t st) {
  const int64_t s = S.s, m = S.m;
  const T *p = S.p, *coef = S.coef;
  if (!seam_ok(S.n, s, m)) return hipErrorInvalidValue;
  const int64_t nlines = S.n / m;
  if (s > 1) {
    hipLaunchKernelGGL((seam_stride_kernel<T, 1>), line_grid(nlines), dim3(256), 0, st, nlines, s, m, p, coef, r);
    return hipGetLastError();
  }
#define SEAMX(W)                                                                                                       \
  hipLaunchKernelGGL((seamx_kernel<W, T>), line_grid((nlines + 64 / W - 1) / (64 / W) * 64), dim3(256), 0, st, nlines, \
                     m, p, coef, r)
  if (m <= 4) SEAMX(4);
  else if (m <= 8) SEAMX(8);
  else if (m <= 16) SEAMX(16);
  else if (m <= 32) SEAMX(32);
  else SEAMX(64);
#undef SEAMX
  return hipGetLastError();
}
}  // namespace
hipError_t launch_line_seam(const SeamRef& S, double* r, hipStream_t st) { return line_seam_t(S, r, st); }
hipError_t launch_line_seam_f32(const SeamRefT<float>& S, float* r, hipStream_t st) { return line_seam_t(S, r, st); }

// ---- K-LineBlock: the line smoothers on the panels of K-Block (kernels.hpp) ---------------------
// Row-major n x KP panels; the factor arrays are the single-vector ones, indexed by row.  K-Line and
// the strided seams are their own kernels at KP > 1 (line_*_kernel<T, KP>, seam_stride_kernel<T, KP>).
// The x direction keeps kernels of its own, because the panel makes it a different algorithm (a
// merge with linex_kernel / seamx_kernel would only add branches); per (row, column) they still
// evaluate the expressions of the single-vector kernel in the same order, so column j has its bits:
//   block_linex_fwd / _bwd      linex_kernel<LX_FWD / LX_BWD>, lane = (run, column): an x line has
//                               stride KP in the panel, so the KP columns of a step are one segment
//                               and the walk needs no transposition through LDS; the rows of the
//                               next LINEXB_BATCH steps are loaded before this batch is walked
//   block_seamx                 seamx_kernel, lane = (line, column): the butterfly as seen from one lane
namespace {
constexpr int LINEXB_BATCH = 8;
// y_i = (r_i - dl_i y_(i-1)) ip_i over the rows [run len, run len + len) below n, in place
template <int KP>
__global__ __launch_bounds__(64) void block_linex_fwd_kernel(int64_t n, int64_t len, int64_t nruns, double* r,
                                                             const double* __restrict__ dl,
                                                             const double* __restrict__ ip) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t run = t / KP;
  const int j = (int)(t % KP);
  if (run >= nruns) return;
  const int64_t i0 = run * len;
  const int64_t cnt = n - i0 < len ? n - i0 : len;
  double ra[LINEXB_BATCH], rb[LINEXB_BATCH], rc[LINEXB_BATCH];
  auto fetch = [&](int64_t k0) {
#pragma unroll
    for (int q = 0; q < LINEXB_BATCH; ++q) {
      const int64_t i = i0 + k0 + q;
      const bool on = k0 + q < cnt;
      ra[q] = on ? r[i * KP + j] : 0.0;
      rb[q] = on ? dl[i] : 0.0;
      rc[q] = on ? ip[i] : 0.0;
    }
  };
  double carry = 0.0;
  fetch(0);
  for (int64_t k0 = 0; k0 < cnt; k0 += LINEXB_BATCH) {
    double a[LINEXB_BATCH], b[LINEXB_BATCH], c[LINEXB_BATCH];
#pragma unroll
    for (int q = 0; q < LINEXB_BATCH; ++q) {
      a[q] = ra[q];
      b[q] = rb[q];
      c[q] = rc[q];
    }
    if (k0 + LINEXB_BATCH < cnt) fetch(k0 + LINEXB_BATCH);
#pragma unroll
    for (int q = 0; q < LINEXB_BATCH; ++q) {
      if (k0 + q < cnt) {
        carry = (a[q] - b[q] * carry) * c[q];
        r[(i0 + k0 + q) * KP + j] = carry;
      }
    }
  }
}
// x_i = y_i - cp_i x_(i+1); u_i += omega x_i, the run's rows descending
template <int KP>
__global__ __launch_bounds__(64) void block_linex_bwd_kernel(int64_t n, int64_t len, int64_t nruns,
                                                             const double* __restrict__ y,
                                                             const double* __restrict__ cp, double* u, double omega) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t run = t / KP;
  const int j = (int)(t % KP);
  if (run >= nruns) return;
  const int64_t i0 = run * len;
  const int64_t cnt = n - i0 < len ? n - i0 : len;
  double ra[LINEXB_BATCH], rb[LINEXB_BATCH], rc[LINEXB_BATCH];
  auto fetch = [&](int64_t k0) {
#pragma unroll
    for (int q = 0; q < LINEXB_BATCH; ++q) {
      const int64_t i = i0 + k0 + q;
      const bool on = k0 + q < cnt;
      ra[q] = on ? y[i * KP + j] : 0.0;
      rb[q] = on ? cp[i] : 0.0;
      rc[q] = on ? u[i * KP + j] : 0.0;
    }
  };
  double carry = 0.0;
  const int64_t last = (cnt - 1) / LINEXB_BATCH * LINEXB_BATCH;  // first row of the last batch (cnt >= 1)
  fetch(last);
  for (int64_t k0 = last; k0 >= 0; k0 -= LINEXB_BATCH) {
    double a[LINEXB_BATCH], b[LINEXB_BATCH], c[LINEXB_BATCH];
#pragma unroll
    for (int q = 0; q < LINEXB_BATCH; ++q) {
      a[q] = ra[q];
      b[q] = rb[q];
      c[q] = rc[q];
    }
    if (k0 > 0) fetch(k0 - LINEXB_BATCH);
#pragma unroll
    for (int q = LINEXB_BATCH - 1; q >= 0; --q) {
      if (k0 + q < cnt) {
        carry = a[q] - b[q] * carry;
        u[(i0 + k0 + q) * KP + j] = c[q] + omega * carry;
      }
    }
  }
}

// x lines: the W partial sums of seamx_kernel<W> (columns l, l + W, ... ascending) formed by the one
// lane, then its butterfly as seen from lane 0: off = W / 2 .. 1, part[l] += part[l + off]
template <int W>
__global__ __launch_bounds__(256) void block_seamx_kernel(int64_t nlines, int64_t m, int kp,
                                                          const double* __restrict__ p,
                                                          const double* __restrict__ coef, double* r) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t line = t / kp;
  const int j = (int)(t % kp);
  if (line >= nlines) return;
  const int64_t i0 = line * m;
  double part[W];
#pragma unroll
  for (int l = 0; l < W; ++l) part[l] = 0.0;
  for (int64_t c0 = 0; c0 < m; c0 += W) {
#pragma unroll
    for (int l = 0; l < W; ++l)
      if (c0 + l < m) part[l] = part[l] + p[i0 + c0 + l] * r[(i0 + c0 + l) * kp + j];
  }
#pragma unroll
  for (int off = W / 2; off >= 1; off >>= 1) {
#pragma unroll
    for (int l = 0; l < off; ++l) part[l] = part[l] + part[l + off];
  }
  const double fac = part[0] / coef[line];
  const int64_t e0 = i0 * kp + j, e1 = (i0 + m - 1) * kp + j;
  r[e0] = r[e0] - fac * coef[nlines + line];
  r[e1] = r[e1] - fac * coef[2 * nlines + line];
}
}  // namespace

hipError_t launch_block_linex_solve(int kp, const LineXRef& L, double* r, double* u, double omega, hipStream_t st) {
  if (!block_kp_ok(kp) || !linex_ok(L)) return hipErrorInvalidValue;
  const int64_t n = L.n, len = linex_run(L.nx), nruns = (n + len - 1) / len;
  const dim3 grid = line_grid(nruns * kp, 64);
#define AMG_BLOCK_LINEX(KP)                                                                                      \
  hipLaunchKernelGGL(block_linex_fwd_kernel<KP>, grid, dim3(64), 0, st, n, len, nruns, r, L.dl, L.ip);           \
  hipLaunchKernelGGL(block_linex_bwd_kernel<KP>, grid, dim3(64), 0, st, n, len, nruns, (const double*)r, L.cp, u, \
                     omega)
  AMG_BLOCK_KP(kp, AMG_BLOCK_LINEX)
#undef AMG_BLOCK_LINEX
  return hipGetLastError();
}

hipError_t launch_block_line_seam(int kp, const SeamRef& S, double* r, hipStream_t st) {
  const int64_t n = S.n, s = S.s, m = S.m;
  if (!block_kp_ok(kp) || !seam_ok(n, s, m)) return hipErrorInvalidValue;
  const int64_t nlines = n / m;
  const dim3 grid = line_grid(nlines * kp);
  if (s > 1) {
#define AMG_BLOCK_SEAM(KP) \
  hipLaunchKernelGGL((seam_stride_kernel<double, KP>), grid, dim3(256), 0, st, nlines, s, m, S.p, S.coef, r)
    AMG_BLOCK_KP(kp, AMG_BLOCK_SEAM)
#undef AMG_BLOCK_SEAM
    return hipGetLastError();
  }
#define AMG_BLOCK_SEAMX(W) \
  hipLaunchKernelGGL(block_seamx_kernel<W>, grid, dim3(256), 0, st, nlines, m, kp, S.p, S.coef, r)
  if (m <= 4) AMG_BLOCK_SEAMX(4);
  else if (m <= 8) AMG_BLOCK_SEAMX(8);
  else if (m <= 16) AMG_BLOCK_SEAMX(16);
  else if (m <= 32) AMG_BLOCK_SEAMX(32);
  else AMG_BLOCK_SEAMX(64);
#undef AMG_BLOCK_SEAMX
  return hipGetLastError();
}
#undef AMG_BLOCK_KP

// ------------------------------------------------------------------ K-F32 ----
// The single-precision preconditioner (solver.cpp: "fp32 cycle"): the V-cycle's row kernels on
// float vectors and float matrix values.  The outer PCG stays in double; nothing here is bitwise
// against the double kernels, only deterministic.
//
// sell_f32_kernel: sell_kernel's walk (one lane per storage row, panel offsets and 16- or 32-bit
// indices SHARED with the double matrix, ascending column order, all loads of a pass issued before
// the first use) with x, f, out, d and the values in float: a wave's value load is one 256-B
// segment, its 16-bit index load one 128-B line.  Modes CSR_RESID, CSR_JACOBI and the Chebyshev
// steps; no non-temporal form.
template <int MODE>
__device__ __forceinline__ float cheb_update_f32(float t, float xi, float di, float alpha, float beta, float& dn) {
  const float z = t - xi;
  dn = cheb_first(MODE) ? beta * z : alpha * di + beta * z;
  return xi + dn;
}
template <int MODE>
__device__ __forceinline__ void f32_row_epilogue(int64_t row, float fi, float xi, float di, float acc, float diag,
                                                 float omega, float alpha, float* out, float* dvec) {
  if (MODE == CSR_RESID || MODE == CSR_SPMV) {
    out[row] = acc;
  } else if (MODE == CSR_SPMV_ADD) {
    out[row] = fi + acc;
  } else if (MODE == CSR_JACOBI) {
    out[row] = (diag == 0.0f) ? xi : xi + omega * ((fi - acc) / diag - xi);
  } else {  // Chebyshev step
    float dn;
    out[row] = cheb_update_f32<MODE>((diag == 0.0f) ? xi : (fi - acc) / diag, xi, di, alpha, omega, dn);
    if (!cheb_last(MODE)) dvec[row] = dn;
  }
}

template <int MODE, bool IDX16>
__global__ __launch_bounds__(256) void sell_f32_kernel(
    int n, const int64_t* __restrict__ soff, const void* __restrict__ scol_v, const float* __restrict__ sval,
    const float* x, const float* __restrict__ f, float* out, float omega, float* dvec, float alpha) {
  const int32_t* __restrict__ scol = static_cast<const int32_t*>(scol_v);
  const int16_t* __restrict__ scol16 = static_cast<const int16_t*>(scol_v);
  const int row = blockIdx.x * 256 + threadIdx.x;  // storage row = row
  const int s = row >> 6;
  if ((s << 6) >= n) return;  // whole wave past the end
  const int64_t o0 = soff[s], o1 = soff[s + 1];
  const int w = (int)((o1 - o0) >> 6);  // wave-uniform panel width
  const int64_t base = o0 + (row & 63);
  const bool live = row < n;
  float fi = 0.0f, xi = 0.0f, di = 0.0f;
  if (live) {
    fi = f[row];
    if (mode_jac(MODE)) xi = x[row];
    if (mode_cheb(MODE) && !cheb_first(MODE)) di = dvec[row];
  }
  float acc = (MODE == CSR_RESID) ? fi : 0.0f;
  float diag = 0.0f;
  auto pass = [&](int j0, auto UU) {
    constexpr int UN = decltype(UU)::value;
    int32_t c[UN];
    float v[UN], xx[UN];
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int j = j0 + u < w ? j0 + u : j0;
      const int64_t at = base + ((int64_t)j << 6);
      if (IDX16) {
        const int d = scol16[at];
        c[u] = (d == -32768) ? -1 : row + d;
      } else {
        c[u] = scol[at];
      }
      v[u] = sval[at];
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) xx[u] = x[c[u] >= 0 ? c[u] : 0];
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      if (j0 + u < w && c[u] >= 0) {
        if (MODE == CSR_RESID) {
          acc -= v[u] * xx[u];
        } else {
          if (c[u] == row) diag = v[u];
          else acc += v[u] * xx[u];
        }
      }
    }
  };
  if (w == 0) {  // a panel of empty rows owns no slot (sell_kernel)
  } else if (w <= 3) pass(0, std::integral_constant<int, 3>{});
  else if (w <= 5) pass(0, std::integral_constant<int, 5>{});
  else if (w <= 7) pass(0, std::integral_constant<int, 7>{});
  else if (w <= 9) pass(0, std::integral_constant<int, 9>{});
  else
    for (int j0 = 0; j0 < w; j0 += 8) pass(j0, std::integral_constant<int, 8>{});
  if (live) f32_row_epilogue<MODE>(row, fi, xi, di, acc, diag, omega, alpha, out, dvec);
}

// csr_f32_kernel: plain CSR, one lane per row (the levels SELL would pad by more than a quarter, and
// the CSR transfers P / R of the classical hierarchies: small or irregular matrices).  Modes as
// above plus CSR_SPMV and CSR_SPMV_ADD (f may be out).  rowptr / col are the double matrix's.
template <int MODE>
__global__ __launch_bounds__(256) void csr_f32_kernel(
    int64_t n, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const float* __restrict__ val,
    const float* __restrict__ x, const float* f, float* out, float omega, float* dvec, float alpha) {
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= n) return;
  const int32_t rs = rowptr[row], re = rowptr[row + 1];
  float fi = 0.0f, xi = 0.0f, di = 0.0f;
  if (MODE != CSR_SPMV) fi = f[row];
  if (mode_jac(MODE)) xi = x[row];
  if (mode_cheb(MODE) && !cheb_first(MODE)) di = dvec[row];
  float acc = (MODE == CSR_RESID) ? fi : 0.0f;
  float diag = 0.0f;
  constexpr int U = 4;  // gathers issued together; the sum itself stays in row order
  for (int32_t p = rs; p < re; p += U) {
    int32_t c[U];
    float v[U], xx[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int32_t q = p + u < re ? p + u : p;
      c[u] = col[q];
      v[u] = val[q];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) xx[u] = x[c[u]];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (p + u < re) {
        if (MODE == CSR_RESID) {
          acc -= v[u] * xx[u];
        } else if (mode_jac(MODE)) {
          if ((int64_t)c[u] == row) diag = v[u];
          else acc += v[u] * xx[u];
        } else {
          acc += v[u] * xx[u];
        }
      }
    }
  }
  f32_row_epilogue<MODE>(row, fi, xi, di, acc, diag, omega, alpha, out, dvec);
}

#define AMG_F32_MODES(X)                                             \
  switch (mode) {                                                    \
    case CSR_RESID: X(CSR_RESID); break;                             \
    case CSR_JACOBI: X(CSR_JACOBI); break;                           \
    case cheb_kernel_mode(false, false): X(cheb_kernel_mode(false, false)); break; \
    case cheb_kernel_mode(true, false): X(cheb_kernel_mode(true, false)); break;   \
    case cheb_kernel_mode(false, true): X(cheb_kernel_mode(false, true)); break;   \
    case cheb_kernel_mode(true, true): X(cheb_kernel_mode(true, true)); break;     \
    default: return hipErrorInvalidValue;                            \
  }

hipError_t launch_sell_f32(int mode, int64_t n, int idx16, const int64_t* soff, const void* scol, const float* sval,
                           const float* x, const float* f, float* out, float omega, float* dvec, float alpha,
                           hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (n >= ((int64_t)1 << 31) - 256 || x == out) return hipErrorInvalidValue;
  if (mode_cheb(mode) && !dvec) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((n + 255) / 256));
#define AMG_F32_SELL(M)                                                                                          \
  if (idx16 & 1)                                                                                                 \
    hipLaunchKernelGGL((sell_f32_kernel<M, true>), grid, dim3(256), 0, st, (int)n, soff, scol, sval, x, f, out,  \
                       omega, dvec, alpha);                                                                      \
  else                                                                                                           \
    hipLaunchKernelGGL((sell_f32_kernel<M, false>), grid, dim3(256), 0, st, (int)n, soff, scol, sval, x, f, out, \
                       omega, dvec, alpha)
  AMG_F32_MODES(AMG_F32_SELL)
#undef AMG_F32_SELL
  return hipGetLastError();
}

hipError_t launch_csr_f32(int mode, int64_t n, const int32_t* rowptr, const int32_t* col, const float* val,
                          const float* x, const float* f, float* out, float omega, float* dvec, float alpha,
                          hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (x == out) return hipErrorInvalidValue;
  if (mode_cheb(mode) && !dvec) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((n + 255) / 256));
#define AMG_F32_CSR(M) \
  hipLaunchKernelGGL((csr_f32_kernel<M>), grid, dim3(256), 0, st, n, rowptr, col, val, x, f, out, omega, dvec, alpha)
  switch (mode) {
    case CSR_SPMV: AMG_F32_CSR(CSR_SPMV); return hipGetLastError();
    case CSR_SPMV_ADD: AMG_F32_CSR(CSR_SPMV_ADD); return hipGetLastError();
  }
  AMG_F32_MODES(AMG_F32_CSR)
#undef AMG_F32_CSR
  return hipGetLastError();
}

// dict_f32_kernel (K-DictF32): dict_kernel's plain path (dict_fetch / dict_expand / dict_rows /
// dict_store) on float vectors.  The matrix is the DOUBLE matrix's own: code words or row types with
// their word table, the pair table's column offsets, the typed / untyped choice; the only float array
// is the pair table's values, tabv[t] = (float)dval[t].  LDS: one 16-byte entry per code {a, d, off4}
// (off4 = BYTE offset of the column from the row's diagonal column in a float vector; entry 255 = no
// entry = all zero, its gather reads the row's own x) and the word table of the double kernel.
// Arithmetic = tests/f32_twin.py: a row's entries in code order (ascending column), every product
// rounded on its own (no contraction), CSR_RESID from f_i with empty slots dropped by a select (acc -
// (+0.0f) == acc for every acc), Jacobi / Chebyshev from +0.0f over the off-diagonal entries with
// (+0.0f) * x added for the diagonal slot and for empty slots as dict_rows does in double, the diagonal
// from the d column, f32_row_epilogue's expressions.  CONDITION: finite vectors.  For finite x the
// added term is +-0.0f, and a sum that starts at +0.0f never becomes -0.0f, so the result has the bits
// of skipping the slot; an infinite or NaN x in the row's own column would turn the row into NaN where
// the SELL / CSR float kernels do not read it.
// R rows per lane (2: 8-byte lane accesses of x, f, d, out and 16-bit row-type loads; 4: 16-byte
// accesses and 32-bit row-type loads); a lane whose R rows are not all below n takes them one at a
// time.  The gathers of at most G rows are in flight together (two-word rows: 2).  No wave-uniform
// stencil path, no non-temporal accesses, no fused forms.
struct __attribute__((aligned(16))) DictEntryF32 {
  float a;
  float d;
  int32_t off4;
  int32_t pad;
};
template <int MODE, int WORDS, int UN, int R>
__global__ __launch_bounds__(256) void dict_f32_kernel(
    int n, const uint64_t* __restrict__ codes, const uint8_t* __restrict__ rtype,
    const uint64_t* __restrict__ rwords, const int32_t* __restrict__ doff, const float* __restrict__ tabv,
    int ntab, const float* x, const float* __restrict__ f, float* out, float omega, int xcd_map, float* dvec,
    float alpha) {
  static_assert(R == 2 || R == 4, "rows per lane");
  typedef float fvec __attribute__((ext_vector_type(R)));
  typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));
  constexpr bool jac = mode_jac(MODE);
  constexpr bool read_d = mode_cheb(MODE) && !cheb_first(MODE);
  __shared__ DictEntryF32 tab[256];
  __shared__ uint64_t wtab[256 * WORDS];
  const int row0 = (xcd_tile(blockIdx.x, gridDim.x, xcd_map) * 256 + (int)threadIdx.x) * R;
  // ---- the streamed operands: in flight while the tables are staged
  uint64_t cw[R][WORDS];
  uint32_t ty = 0xFFFFFFFFu;  // byte r = type of row r, 255 = empty
  float fi[R], xi[R], di[R];
  bool live[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    live[r] = row0 + r < n;
    fi[r] = xi[r] = di[r] = 0.0f;
#pragma unroll
    for (int k = 0; k < WORDS; ++k) cw[r][k] = ~(uint64_t)0;
  }
  const bool full = live[R - 1];
  if (full) {
    if (rtype) {  // wave-uniform
      if (R == 4) ty = *reinterpret_cast<const uint32_t*>(rtype + row0);
      else ty = 0xFFFF0000u | *reinterpret_cast<const uint16_t*>(rtype + row0);
    } else {
      const u64x2* vp = reinterpret_cast<const u64x2*>(codes + (int64_t)row0 * WORDS);
#pragma unroll
      for (int q = 0; q < R * WORDS / 2; ++q) {
        const u64x2 t = vp[q];
        cw[(2 * q) / WORDS][(2 * q) % WORDS] = t.x;
        cw[(2 * q + 1) / WORDS][(2 * q + 1) % WORDS] = t.y;
      }
    }
    const fvec tf = *reinterpret_cast<const fvec*>(f + row0);
#pragma unroll
    for (int r = 0; r < R; ++r) fi[r] = tf[r];
    if (jac) {
      const fvec tx = *reinterpret_cast<const fvec*>(x + row0);
#pragma unroll
      for (int r = 0; r < R; ++r) xi[r] = tx[r];
    }
    if (read_d) {
      const fvec td = *reinterpret_cast<const fvec*>(dvec + row0);
#pragma unroll
      for (int r = 0; r < R; ++r) di[r] = td[r];
    }
  } else {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (!live[r]) continue;
      if (rtype) {
        ty = (ty & ~(0xFFu << (8 * r))) | ((uint32_t)rtype[row0 + r] << (8 * r));
      } else {
#pragma unroll
        for (int k = 0; k < WORDS; ++k) cw[r][k] = codes[(int64_t)(row0 + r) * WORDS + k];
      }
      fi[r] = f[row0 + r];
      if (jac) xi[r] = x[row0 + r];
      if (read_d) di[r] = dvec[row0 + r];
    }
  }
  // ---- the tables
  {
    const int t = threadIdx.x;  // 256 threads, 256 entries
    const float v = t < ntab ? tabv[t] : 0.0f;
    const int32_t o = t < ntab ? doff[t] : 0;
    DictEntryF32 e;
    e.a = (jac && o == 0) ? 0.0f : v;
    e.d = (jac && o == 0 && t < ntab) ? v : 0.0f;
    e.off4 = o * 4;
    e.pad = 0;
    tab[t] = e;
  }
  if (rtype) dict_stage_words<WORDS>(wtab, rwords);
  __syncthreads();
  if (rtype) {
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int k = 0; k < WORDS; ++k) cw[r][k] = wtab[((ty >> (8 * r)) & 0xFFu) * WORDS + k];
  }
  // ---- decode, gather, row arithmetic: G rows at a time
  constexpr int G = (WORDS == 2 && R > 2) ? 2 : R;
  const char* xb = reinterpret_cast<const char*>(x);
  float res[R], dn[R];
#pragma unroll
  for (int g0 = 0; g0 < R; g0 += G) {
    uint32_t c4[G][UN];
    float v[G][UN], vd[G][UN], xx[G][UN];
    bool ok[G][UN];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const int r = g0 + g;
      const uint32_t drow4 = live[r] ? (uint32_t)(row0 + r) * 4u : 0u;
#pragma unroll
      for (int u = 0; u < UN; ++u) {
        const uint32_t w32 = (uint32_t)(cw[r][u >> 3] >> (32 * ((u >> 2) & 1)));
        const uint32_t code = (w32 >> (8 * (u & 3))) & 0xFFu;
        const DictEntryF32 e = tab[code];
        ok[g][u] = code != 0xFFu;
        c4[g][u] = drow4 + (uint32_t)e.off4;
        v[g][u] = e.a;
        vd[g][u] = jac ? e.d : 0.0f;
      }
    }
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int u = 0; u < UN; ++u) xx[g][u] = *reinterpret_cast<const float*>(xb + c4[g][u]);
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const int r = g0 + g;
      float acc = (MODE == CSR_RESID) ? fi[r] : 0.0f;
      float diag = 0.0f;
#pragma unroll
      for (int u = 0; u < UN; ++u) {
        float t = v[g][u] * xx[g][u];
        if (jac) {
          acc += t;
          diag += vd[g][u];
        } else {
          asm volatile("" : "+v"(t));  // keeps the product and its gather out of a branch (dict_rows)
          t = ok[g][u] ? t : 0.0f;
          acc -= t;
        }
      }
      if (MODE == CSR_RESID) {
        res[r] = acc;
      } else {
        // f32_row_epilogue's expressions; the division runs for every row (dict_rows)
        const bool nod = diag == 0.0f;
        float q = (fi[r] - acc) / (nod ? 1.0f : diag);
        asm volatile("" : "+v"(q));
        if (MODE == CSR_JACOBI) res[r] = nod ? xi[r] : xi[r] + omega * (q - xi[r]);
        else res[r] = cheb_update_f32<MODE>(nod ? xi[r] : q, xi[r], di[r], alpha, omega, dn[r]);
      }
    }
  }
  // ---- store
  constexpr bool write_d = mode_cheb(MODE) && !cheb_last(MODE);
  if (full) {
    fvec t;
#pragma unroll
    for (int r = 0; r < R; ++r) t[r] = res[r];
    *reinterpret_cast<fvec*>(out + row0) = t;
    if (write_d) {
#pragma unroll
      for (int r = 0; r < R; ++r) t[r] = dn[r];
      *reinterpret_cast<fvec*>(dvec + row0) = t;
    }
  } else {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (!live[r]) continue;
      out[row0 + r] = res[r];
      if (write_d) dvec[row0 + r] = dn[r];
    }
  }
}

// Rows per lane of dict_f32_kernel: DICT_F32_ROWS, the faster one on the level-0 sweep of
// poisson_tensor(4096) (66 us against 84 us with 4; DESIGN.md: "Single-precision preconditioner");
// set_dict_rows_per_lane(1), the test switch of the double kernels, selects the other one.  Same bits
// either way.
constexpr int DICT_F32_ROWS = 2;
static int dict_f32_rows() { return g_dict_rows_per_lane == 1 ? 6 - DICT_F32_ROWS : DICT_F32_ROWS; }
hipError_t launch_dict_f32(int mode, int64_t n, const DictRef& D, const float* tabv, const float* x, const float* f,
                           float* out, float omega, float* dvec, float alpha, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  // byte offsets of x are 32-bit: 4 (n + 1024) < 2^32
  if (!dict_args_ok(n, D.words, D.wmax, D.ntab) || n >= ((int64_t)1 << 30) - 1024 || x == out || !tabv)
    return hipErrorInvalidValue;
  if (mode_cheb(mode) && !dvec) return hipErrorInvalidValue;
  const int R = dict_f32_rows();
  const uintptr_t vec = reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(f) |
                        reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(dvec);
  if ((vec & (uintptr_t)(4 * R - 1)) != 0) return hipErrorInvalidValue;
  if (D.rtype ? (reinterpret_cast<uintptr_t>(D.rtype) & (uintptr_t)(R - 1)) != 0
              : (reinterpret_cast<uintptr_t>(D.codes) & 15) != 0)
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)((n + 256 * R - 1) / (256 * R)));
  const int xcd = dict_xcd_map(D, 256 * R);
#define AMG_F32_DICT_WU(M, W, U)                                                                                  \
  do {                                                                                                            \
    if (R == 4)                                                                                                   \
      hipLaunchKernelGGL((dict_f32_kernel<M, W, U, 4>), grid, dim3(256), 0, st, (int)n, D.codes, D.rtype, D.rwords, \
                         D.doff, tabv, D.ntab, x, f, out, omega, xcd, dvec, alpha);                               \
    else                                                                                                          \
      hipLaunchKernelGGL((dict_f32_kernel<M, W, U, 2>), grid, dim3(256), 0, st, (int)n, D.codes, D.rtype, D.rwords, \
                         D.doff, tabv, D.ntab, x, f, out, omega, xcd, dvec, alpha);                               \
  } while (0)
#define AMG_F32_DICT(M)                                     \
  if (D.words == 1) {                                       \
    if (D.wmax <= 5) AMG_F32_DICT_WU(M, 1, 5);              \
    else if (D.wmax <= 7) AMG_F32_DICT_WU(M, 1, 7);         \
    else AMG_F32_DICT_WU(M, 1, 8);                          \
  } else {                                                  \
    if (D.wmax <= 9) AMG_F32_DICT_WU(M, 2, 9);              \
    else AMG_F32_DICT_WU(M, 2, 16);                         \
  }
  AMG_F32_MODES(AMG_F32_DICT)
#undef AMG_F32_DICT
#undef AMG_F32_DICT_WU
  return hipGetLastError();
}
#undef AMG_F32_MODES

// double <-> float, four entries per lane: 16-byte lane accesses on the float side and on both
// halves of the double side when both pointers are 16-byte aligned (VEC), else one entry per lane.
template <bool VEC>
__global__ __launch_bounds__(256) void to_f32_kernel(int64_t n, const double* __restrict__ src,
                                                     float* __restrict__ dst) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (!VEC) {
    if (t < n) dst[t] = (float)src[t];
    return;
  }
  const int64_t i = 4 * t;
  if (i + 3 < n) {
    const double2 a = *reinterpret_cast<const double2*>(src + i);
    const double2 b = *reinterpret_cast<const double2*>(src + i + 2);
    *reinterpret_cast<float4*>(dst + i) = make_float4((float)a.x, (float)a.y, (float)b.x, (float)b.y);
  } else {
    for (int64_t k = i; k < n; ++k) dst[k] = (float)src[k];
  }
}
template <bool VEC>
__global__ __launch_bounds__(256) void to_f64_kernel(int64_t n, const float* __restrict__ src,
                                                     double* __restrict__ dst) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (!VEC) {
    if (t < n) dst[t] = (double)src[t];
    return;
  }
  const int64_t i = 4 * t;
  if (i + 3 < n) {
    const float4 a = *reinterpret_cast<const float4*>(src + i);
    *reinterpret_cast<double2*>(dst + i) = make_double2((double)a.x, (double)a.y);
    *reinterpret_cast<double2*>(dst + i + 2) = make_double2((double)a.z, (double)a.w);
  } else {
    for (int64_t k = i; k < n; ++k) dst[k] = (double)src[k];
  }
}
__global__ __launch_bounds__(256) void zero_f32_kernel(int64_t n, float* __restrict__ x) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) x[i] = 0.0f;
}
hipError_t launch_zero_f32(int64_t n, float* x, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(zero_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, x);
  return hipGetLastError();
}
hipError_t launch_to_f32(int64_t n, const double* src, float* dst, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0)
    hipLaunchKernelGGL(to_f32_kernel<true>, dim3((unsigned)(((n + 3) / 4 + 255) / 256)), dim3(256), 0, st, n, src, dst);
  else
    hipLaunchKernelGGL(to_f32_kernel<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, src, dst);
  return hipGetLastError();
}
hipError_t launch_to_f64(int64_t n, const float* src, double* dst, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0)
    hipLaunchKernelGGL(to_f64_kernel<true>, dim3((unsigned)(((n + 3) / 4 + 255) / 256)), dim3(256), 0, st, n, src, dst);
  else
    hipLaunchKernelGGL(to_f64_kernel<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, src, dst);
  return hipGetLastError();
}

// the float instantiations of the matrix-free transfers (K-Restrict / K-ProlongAdd, K-TensorRestrict /
// K-TensorProlong): same kernels, T = float
hipError_t launch_linear_restrict_f32(int64_t n_h, int64_t n_H, const float* r, float* fH, float* uH_zero,
                                      hipStream_t st) {
  return launch_linear_restrict_t<float>(n_h, n_H, r, fH, uH_zero, st);
}
hipError_t launch_linear_prolong_add_f32(int64_t n_h, int64_t n_H, const float* uH, float* uh, hipStream_t st) {
  return launch_linear_prolong_add_t<float>(n_h, n_H, uH, uh, st);
}
hipError_t launch_tensor_restrict_f32(int dim, const int64_t dims[3], uint32_t mask, uint32_t sides, uint32_t periodic, const float* r, float* fH, float* uH_zero,
                                      hipStream_t st) {
  return launch_tensor_restrict_t<float>(dim, dims, mask, sides, periodic, r, fH, uH_zero, st);
}
hipError_t launch_tensor_prolong_add_f32(int dim, const int64_t dims[3], uint32_t mask, uint32_t sides, uint32_t periodic, const float* uH, float* uh,
                                         hipStream_t st) {
  return launch_tensor_prolong_add_t<float>(dim, dims, mask, sides, periodic, uH, uh, st);
}


}  // namespace amg_hip
