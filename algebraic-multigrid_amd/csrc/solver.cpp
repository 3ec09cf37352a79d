// =============================================================================
// solver.cpp -- the C ABI of include/amg_hip.h: solver handle, V-cycle
// orchestration on one HIP stream (replayed as a hipGraph), stand-alone plug-in
// operations and device-pointer launchers.  No CPU fallback anywhere: every
// compute entry point needs a HIP device and fails with AMG_HIP_EHIP otherwise.
// =============================================================================
#include <cstddef>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include <dlfcn.h>

#include "../../include/amg_hip.h"
#include "capture_once.hpp"
#include "host_setup.hpp"
#include "kernels.hpp"

using namespace amg_hip;
#ifdef AMG_PATCH_STAMPS
namespace amg_hip {
hipError_t debug_set_patch_stamps(unsigned long long* p);
hipError_t debug_set_patch_stamps_rows(int rows);
}
#endif

namespace {

thread_local std::string g_err;

amg_hip_status fail(amg_hip_status st, const std::string& msg) {
  g_err = msg;
  return st;
}

#define HIP_TRY(expr)                                                          \
  do {                                                                         \
    hipError_t _e = (expr);                                                    \
    if (_e != hipSuccess)                                                      \
      return fail(_e == hipErrorOutOfMemory ? AMG_HIP_ENOMEM : AMG_HIP_EHIP,   \
                  std::string(#expr) + ": " + hipGetErrorString(_e));          \
  } while (0)
#define AMG_TRY(expr)                                                          \
  do {                                                                         \
    const amg_hip_status _s = (expr);                                          \
    if (_s != AMG_HIP_OK) return _s;                                           \
  } while (0)

int host_threads() {
  unsigned h = std::thread::hardware_concurrency();
  if (h == 0) h = 1;
  return (int)std::min(h, 16u);
}

// ---- device buffers ---------------------------------------------------------
struct DevMem {  // owns one hipMalloc allocation
  void* p = nullptr;
  size_t bytes = 0;
  DevMem() = default;
  DevMem(const DevMem&) = delete;
  DevMem& operator=(const DevMem&) = delete;
  DevMem(DevMem&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
  DevMem& operator=(DevMem&& o) noexcept {
    if (this != &o) { release(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; }
    return *this;
  }
  ~DevMem() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  // 64 bytes of slack so that 16-byte vector loads of a tail never leave the
  // allocation
  hipError_t alloc(size_t n) {
    release();
    bytes = n;
    return hipMalloc(&p, n + 64);
  }
  template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

template <class T>
hipError_t upload(DevMem& m, const T* src, size_t count) {
  hipError_t e = m.alloc(count * sizeof(T));
  if (e != hipSuccess) return e;
  if (count == 0) return hipSuccess;
  return hipMemcpy(m.p, src, count * sizeof(T), hipMemcpyHostToDevice);
}

struct DevCsr {  // row-major view on the device
  int64_t n_rows = 0, n_cols = 0, nnz = 0;
  int max_block_nnz = 0, max_row_nnz = 0;
  DevMem ptr, idx, val;
  const int32_t* rowptr() const { return ptr.as<int32_t>(); }
  const int32_t* col() const { return idx.as<int32_t>(); }
  const double* v() const { return val.as<double>(); }
};

// The square CSR matrix of n rows behind three device pointers, copied to the host on the stream
// `st`; the number of entries is read from the row pointers, and an empty matrix copies only those.
hipError_t download_csr(int64_t n, const int32_t* ptr, const int32_t* idx, const double* val, hipStream_t st,
                        Sparse* H) {
  H->n_outer = H->n_inner = n;
  H->ptr.resize((size_t)n + 1);
  hipError_t e = hipMemcpyAsync(H->ptr.data(), ptr, sizeof(int32_t) * H->ptr.size(), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return e;
  const size_t nnz = (size_t)H->ptr.back();
  H->idx.resize(nnz);
  H->val.resize(nnz);
  if (nnz == 0) return hipSuccess;
  e = hipMemcpyAsync(H->idx.data(), idx, sizeof(int32_t) * nnz, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(H->val.data(), val, sizeof(double) * nnz, hipMemcpyDeviceToHost, st);
  return e == hipSuccess ? hipStreamSynchronize(st) : e;
}
hipError_t download_csr(const DevCsr& A, Sparse* H) {
  return download_csr(A.n_rows, A.rowptr(), A.col(), A.v(), nullptr, H);
}

void csr_shape(const Sparse& M, int* max_block, int* max_row) {
  int mb = 0, mr = 0;
  for (int64_t r = 0; r < M.n_outer; ++r) mr = std::max(mr, M.ptr[r + 1] - M.ptr[r]);
  for (int64_t r = 0; r < M.n_outer; r += 256) {
    const int64_t e = std::min<int64_t>(r + 256, M.n_outer);
    mb = std::max(mb, M.ptr[e] - M.ptr[r]);
  }
  *max_block = mb;
  *max_row = mr;
}

hipError_t upload_csr(const Sparse& M, DevCsr* D) {
  D->n_rows = M.n_outer;
  D->n_cols = M.n_inner;
  D->nnz = M.nnz();
  csr_shape(M, &D->max_block_nnz, &D->max_row_nnz);
  hipError_t e;
  if ((e = upload(D->ptr, M.ptr.data(), M.ptr.size())) != hipSuccess) return e;
  if ((e = upload(D->idx, M.idx.data(), M.idx.size())) != hipSuccess) return e;
  return upload(D->val, M.val.data(), M.val.size());
}

// Setup on the device (K-Galerkin): AH = R (A P) for the linear interpolation pair from
// CSR(A) that already sits on the device; AH stays there for the next level and is
// copied to the host (the hierarchy's host copy, layout encoding, getters).
hipError_t device_galerkin(const DevCsr& A, int64_t n_H, DevCsr* AH, Sparse* host) {
  const int64_t n_h = A.n_rows;
  hipError_t e;
  DevMem cnt, bsum, total, ap_ptr, ap_idx, ap_val;
  const int64_t nmax = std::max(n_h, n_H);
  if ((e = cnt.alloc(sizeof(int32_t) * (nmax + 1))) != hipSuccess) return e;
  if ((e = bsum.alloc(sizeof(int64_t) * ((nmax + 1023) / 1024 + 1))) != hipSuccess) return e;
  if ((e = total.alloc(sizeof(int64_t))) != hipSuccess) return e;
  auto scan = [&](int64_t n, DevMem& ptr, int64_t* tot) -> hipError_t {
    hipError_t q;
    if ((q = ptr.alloc(sizeof(int32_t) * (n + 1))) != hipSuccess) return q;
    if ((q = launch_exclusive_scan(n, cnt.as<int32_t>(), ptr.as<int32_t>(), bsum.as<int64_t>(),
                                   total.as<int64_t>(), nullptr)) != hipSuccess)
      return q;
    return hipMemcpy(tot, total.p, sizeof(int64_t), hipMemcpyDeviceToHost);
  };
  // A P
  if ((e = launch_galerkin_ap(false, n_h, n_H, A.rowptr(), A.col(), A.v(), cnt.as<int32_t>(),
                              nullptr, nullptr, nullptr, nullptr)) != hipSuccess)
    return e;
  int64_t nnz_ap = 0;
  if ((e = scan(n_h, ap_ptr, &nnz_ap)) != hipSuccess) return e;
  if (nnz_ap >= ((int64_t)1 << 31) - 1) return hipErrorInvalidValue;
  if ((e = ap_idx.alloc(sizeof(int32_t) * std::max<int64_t>(nnz_ap, 1))) != hipSuccess) return e;
  if ((e = ap_val.alloc(sizeof(double) * std::max<int64_t>(nnz_ap, 1))) != hipSuccess) return e;
  if ((e = launch_galerkin_ap(true, n_h, n_H, A.rowptr(), A.col(), A.v(), nullptr,
                              ap_ptr.as<int32_t>(), ap_idx.as<int32_t>(), ap_val.as<double>(),
                              nullptr)) != hipSuccess)
    return e;
  // R (A P)
  if ((e = launch_galerkin_rap(false, n_h, n_H, ap_ptr.as<int32_t>(), ap_idx.as<int32_t>(),
                               ap_val.as<double>(), cnt.as<int32_t>(), nullptr, nullptr, nullptr,
                               nullptr)) != hipSuccess)
    return e;
  int64_t nnz = 0;
  if ((e = scan(n_H, AH->ptr, &nnz)) != hipSuccess) return e;
  if (nnz >= ((int64_t)1 << 31) - 1) return hipErrorInvalidValue;
  if ((e = AH->idx.alloc(sizeof(int32_t) * std::max<int64_t>(nnz, 1))) != hipSuccess) return e;
  if ((e = AH->val.alloc(sizeof(double) * std::max<int64_t>(nnz, 1))) != hipSuccess) return e;
  if ((e = launch_galerkin_rap(true, n_h, n_H, ap_ptr.as<int32_t>(), ap_idx.as<int32_t>(),
                               ap_val.as<double>(), nullptr, AH->ptr.as<int32_t>(),
                               AH->idx.as<int32_t>(), AH->val.as<double>(), nullptr)) != hipSuccess)
    return e;
  AH->n_rows = AH->n_cols = n_H;
  AH->nnz = nnz;
  if (!host) return hipSuccess;  // device-only setup: the host copy is made when a getter asks
  host->n_outer = host->n_inner = n_H;
  host->ptr.resize(n_H + 1);
  host->idx.resize(nnz);
  host->val.resize(nnz);
  if ((e = hipMemcpy(host->ptr.data(), AH->ptr.p, sizeof(int32_t) * (n_H + 1), hipMemcpyDeviceToHost)) != hipSuccess) return e;
  if (nnz > 0) {
    if ((e = hipMemcpy(host->idx.data(), AH->idx.p, sizeof(int32_t) * nnz, hipMemcpyDeviceToHost)) != hipSuccess) return e;
    if ((e = hipMemcpy(host->val.data(), AH->val.p, sizeof(double) * nnz, hipMemcpyDeviceToHost)) != hipSuccess) return e;
  }
  return hipSuccess;
}

// Setup on the device (K-TensorGalerkin): AH = R (A P) for the tensor-product pair of the grid
// `dims` (mask: the coarsened axes, sides: the natural boundary sides, periodic: the periodic axes)
// from CSR(A) on the device.  *ok = false: a coarse row reaches more columns than the
// kernel's lane group holds; hipErrorInvalidValue: the product is beyond int32 indexing.  Either
// way the caller takes the host path.
// axis >= 0 (mask = 1 << axis): the one-axis pair with the weights W on the device (K-AxisGalerkin)
// instead of the tensor-product pair; `periodic` then selects its seam form (sides: not used).
hipError_t device_tensor_galerkin(const DevCsr& A, int dim, const int64_t dims[3], uint32_t mask, uint32_t sides,
                                  uint32_t periodic, int64_t n_H,
                                  DevCsr* AH,
                                  bool* ok, int axis = -1, const double* W = nullptr) {
  *ok = false;
  hipError_t e;
  DevMem cnt, bsum, total, ovf;
  if ((e = cnt.alloc(sizeof(int32_t) * (n_H + 1))) != hipSuccess) return e;
  if ((e = bsum.alloc(sizeof(int64_t) * ((n_H + 1023) / 1024 + 1))) != hipSuccess) return e;
  if ((e = total.alloc(sizeof(int64_t))) != hipSuccess) return e;
  if ((e = ovf.alloc(sizeof(int32_t))) != hipSuccess) return e;
  if ((e = hipMemset(ovf.p, 0, sizeof(int32_t))) != hipSuccess) return e;
  e = axis >= 0 ? launch_axis_galerkin(false, dim, dims, axis, periodic, A.rowptr(), A.col(), A.v(), W, cnt.as<int32_t>(), nullptr,
                                       nullptr, nullptr, ovf.as<int32_t>(), nullptr)
                : launch_tensor_galerkin(false, dim, dims, mask, sides, periodic, A.rowptr(), A.col(), A.v(), cnt.as<int32_t>(), nullptr,
                                         nullptr, nullptr, ovf.as<int32_t>(), nullptr);
  if (e != hipSuccess) return e;
  int32_t over = 0;
  if ((e = hipMemcpy(&over, ovf.p, sizeof(int32_t), hipMemcpyDeviceToHost)) != hipSuccess) return e;
  if (over) return hipSuccess;
  if ((e = AH->ptr.alloc(sizeof(int32_t) * (n_H + 1))) != hipSuccess) return e;
  if ((e = launch_exclusive_scan(n_H, cnt.as<int32_t>(), AH->ptr.as<int32_t>(), bsum.as<int64_t>(),
                                 total.as<int64_t>(), nullptr)) != hipSuccess)
    return e;
  int64_t nnz = 0;
  if ((e = hipMemcpy(&nnz, total.p, sizeof(int64_t), hipMemcpyDeviceToHost)) != hipSuccess) return e;
  if (nnz >= ((int64_t)1 << 31) - 1) return hipErrorInvalidValue;
  if ((e = AH->idx.alloc(sizeof(int32_t) * std::max<int64_t>(nnz, 1))) != hipSuccess) return e;
  if ((e = AH->val.alloc(sizeof(double) * std::max<int64_t>(nnz, 1))) != hipSuccess) return e;
  e = axis >= 0 ? launch_axis_galerkin(true, dim, dims, axis, periodic, A.rowptr(), A.col(), A.v(), W, nullptr, AH->ptr.as<int32_t>(),
                                       AH->idx.as<int32_t>(), AH->val.as<double>(), ovf.as<int32_t>(), nullptr)
                : launch_tensor_galerkin(true, dim, dims, mask, sides, periodic, A.rowptr(), A.col(), A.v(), nullptr, AH->ptr.as<int32_t>(),
                                         AH->idx.as<int32_t>(), AH->val.as<double>(), ovf.as<int32_t>(), nullptr);
  if (e != hipSuccess) return e;
  AH->n_rows = AH->n_cols = n_H;
  AH->nnz = nnz;
  *ok = true;
  return hipSuccess;
}

// C = A B on the device (general CSR operands: custom interpolators), count -> scan -> fill.
// *ok = false: a row of A is longer than the kernel's merge width, or an index overflow:
// the caller takes the host product.
hipError_t device_spgemm(const DevCsr& A, const DevCsr& B, DevCsr* C, bool* ok) {
  *ok = false;
  const int64_t n = A.n_rows;
  hipError_t e;
  DevMem cnt, bsum, total, ovf;
  if ((e = cnt.alloc(sizeof(int32_t) * (n + 1))) != hipSuccess) return e;
  if ((e = bsum.alloc(sizeof(int64_t) * ((n + 1023) / 1024 + 1))) != hipSuccess) return e;
  if ((e = total.alloc(sizeof(int64_t))) != hipSuccess) return e;
  if ((e = ovf.alloc(sizeof(int32_t))) != hipSuccess) return e;
  if ((e = hipMemset(ovf.p, 0, sizeof(int32_t))) != hipSuccess) return e;
  if ((e = launch_spgemm(false, n, A.rowptr(), A.col(), A.v(), B.rowptr(), B.col(), B.v(),
                         cnt.as<int32_t>(), nullptr, nullptr, nullptr, ovf.as<int32_t>(), nullptr)) != hipSuccess)
    return e;
  int32_t over = 0;
  if ((e = hipMemcpy(&over, ovf.p, sizeof(int32_t), hipMemcpyDeviceToHost)) != hipSuccess) return e;
  if (over) return hipSuccess;
  if ((e = C->ptr.alloc(sizeof(int32_t) * (n + 1))) != hipSuccess) return e;
  if ((e = launch_exclusive_scan(n, cnt.as<int32_t>(), C->ptr.as<int32_t>(), bsum.as<int64_t>(),
                                 total.as<int64_t>(), nullptr)) != hipSuccess)
    return e;
  int64_t nnz = 0;
  if ((e = hipMemcpy(&nnz, total.p, sizeof(int64_t), hipMemcpyDeviceToHost)) != hipSuccess) return e;
  if (nnz >= ((int64_t)1 << 31) - 1) return hipSuccess;
  if ((e = C->idx.alloc(sizeof(int32_t) * std::max<int64_t>(nnz, 1))) != hipSuccess) return e;
  if ((e = C->val.alloc(sizeof(double) * std::max<int64_t>(nnz, 1))) != hipSuccess) return e;
  if ((e = launch_spgemm(true, n, A.rowptr(), A.col(), A.v(), B.rowptr(), B.col(), B.v(), nullptr,
                         C->ptr.as<int32_t>(), C->idx.as<int32_t>(), C->val.as<double>(),
                         ovf.as<int32_t>(), nullptr)) != hipSuccess)
    return e;
  C->n_rows = n;
  C->n_cols = B.n_cols;
  C->nnz = nnz;
  *ok = true;
  return hipSuccess;
}
// A_H = R (A P) for arbitrary transfer operators (CSR(R), CSR(P) on the device); host copy of
// CSR(A_H) as for device_galerkin
hipError_t device_galerkin_generic(const DevCsr& A, const DevCsr& P, const DevCsr& R, DevCsr* AH,
                                   Sparse* host, bool* ok) {
  DevCsr AP;
  hipError_t e = device_spgemm(A, P, &AP, ok);
  if (e != hipSuccess || !*ok) return e;
  e = device_spgemm(R, AP, AH, ok);
  if (e != hipSuccess || !*ok) return e;
  const int64_t n_H = AH->n_rows, nnz = AH->nnz;
  host->n_outer = host->n_inner = n_H;
  host->ptr.resize(n_H + 1);
  host->idx.resize(nnz);
  host->val.resize(nnz);
  if ((e = hipMemcpy(host->ptr.data(), AH->ptr.p, sizeof(int32_t) * (n_H + 1), hipMemcpyDeviceToHost)) != hipSuccess) return e;
  if (nnz > 0) {
    if ((e = hipMemcpy(host->idx.data(), AH->idx.p, sizeof(int32_t) * nnz, hipMemcpyDeviceToHost)) != hipSuccess) return e;
    if ((e = hipMemcpy(host->val.data(), AH->val.p, sizeof(double) * nnz, hipMemcpyDeviceToHost)) != hipSuccess) return e;
  }
  return hipSuccess;
}

int g_patch_tile_flags = 1;  // amg_hip_set_patch_tile_flags: A/B switch (same bits either way)
int g_axis_stencil = 1;      // amg_hip_set_axis_stencil: A/B switch, read when a solver is created (same bits either way)
int g_patch_xf = 1;          // amg_hip_set_patch_xf: A/B switch (same bits either way)
int g_patch_tall = 1;        // amg_hip_set_patch_tall: A/B switch (same bits either way)
int g_patch_seam = 1;        // amg_hip_set_patch_seam: A/B switch (same bits either way)
int g_patch_coltype = 1;     // amg_hip_set_patch_coltype: A/B switch, read when a solver is created (same bits either way)
// The column-type array beside a flag array of `tiles` tiles (whole words, zero-filled); left empty where the
// switch is off: the flag kernels then build no flag 254.
static hipError_t alloc_patch_ctype(DevMem& ct, int64_t tiles, int rings) {
  ct.release();
  if (!g_patch_coltype) return hipSuccess;
  const hipError_t e = ct.alloc(((size_t)tiles * (size_t)patch_frame_columns(rings) + 3) & ~(size_t)3);
  return e != hipSuccess ? e : hipMemset(ct.p, 0, ct.bytes);
}

// A level matrix on the device in one of the two layouts the kernels take.
struct DevMat {
  bool sell = false;
  int64_t n_rows = 0, nnz = 0;
  DevCsr csr;                 // K-CSR (LDS-staged CSR)
  int max_width = 0;          // K-SELL (64-row panels, lane-interleaved)
  int64_t slots = 0;
  int idx16 = 0;              // scol = int16 offsets from the diagonal column
  DevMem soff, scol, sval;
  bool dict = false;          // K-Dict (dictionary-coded rows)
  int dict_words = 0, dict_wmax = 0, dict_ntab = 0, dict_nt = 0;
  int64_t dict_shift = 0;
  int dict_hb = 0;            // largest |column offset| of the table (half-bandwidth in rows)
  bool dict_typed = false;    // second level: one byte per row into a table of code words
  DevMem dcodes, doff, dval, drtype, drwords;
  DevMem dutd, duti;  // per row type: values / diagonal, offsets + slot mask + stencil pattern (DictRef::utd, uti)
  // K-March (3-D 7-point level: every row type's columns within {-M, -m, -1, 0, 1, m, M}): per type
  // {w(-M), w(-m), w(-1), w(+1), w(+m), w(+M), diagonal, 0}; the interior type and its values
  DevMem dmarch;
  int march_m = 0, march_M = 0, march_ntypes = 0, march_tint = -1;
  double march_wint[6] = {0, 0, 0, 0, 0, 0}, march_dint = 0.0;
  // K-GS-scan: nearest dependency of a lexicographic sweep other than the chained neighbour
  // (min |offset| over the pairs with |offset| >= 2) and the farthest one; 0 = not usable
  int64_t scan_gap = 0, scan_far = 0;
  int scan_new = 99;  // most entries of a row type beyond the chained neighbour on one side
  // K-Patch (temporal blocking): per (row type, slot) table, pitch of the band
  bool patch = false;
  int64_t patch_m = 0;
  int patch_un = 0, patch_ntypes = 0, patch_umask = 0;
  // A tile flag describes the rows a kernel loads for a tile, so there is one array per geometry:
  // patch_flags for the launches with three halo rings (tiles of 42 lines), patch_flags2 for those
  // with two (44 lines), patch_flags5 for the seam launch (five rings in its wider frame, 38 lines;
  // 5-point levels only).  All are built with the matrix (a byte per tile), whichever the level's
  // launches turn out to use.
  DevMem patch_tab, patch_utabd, patch_utabi, patch_flags, patch_flags2, patch_flags5;
  // beside each flag array: the column types of its column-typed tiles (flag 254), a byte per tile and
  // held column (patch_frame_columns(rings)); empty where the switch was off: the flags then hold no 254
  DevMem patch_ctype, patch_ctype2, patch_ctype5;
  // per tile of the level's down-leg (patch_crings rings): the coarse rows under it share the
  // diagonal patch_dH (set_patch_coarse_flags)
  DevMem patch_cflags;
  int patch_crings = 3;
  double patch_dH = 0.0;
  // fraction of the 42-line tiles whose coarse flag is set (bytes accounting: the model is stated
  // on that tiling whatever the tile height of the launch, so it does not move with the geometry)
  double patch_cfrac = 0.0;
  PatchRef patch_ref(int rings = 3) const {
    PatchRef P;
    P.rings = rings;
    P.rtype = drtype.as<uint8_t>();
    P.tflag = g_patch_tile_flags ? (rings == 2 ? patch_flags2 : (rings == 5 ? patch_flags5 : patch_flags)).as<uint8_t>()
                                 : nullptr;
    P.ctype = P.tflag ? (rings == 2 ? patch_ctype2 : (rings == 5 ? patch_ctype5 : patch_ctype)).as<uint8_t>() : nullptr;
    P.cflag = g_patch_tile_flags && rings == patch_crings ? patch_cflags.as<uint8_t>() : nullptr;
    P.dHu = patch_dH;
    P.ptab = patch_tab.as<double>();
    P.utabd = patch_utabd.as<double>();
    P.utabi = patch_utabi.as<int32_t>();
    P.ntypes = patch_ntypes;
    P.un = patch_un;
    P.umask = patch_umask;
    P.nent = patch_ntypes * patch_un;
    P.nt = dict_nt;
    return P;
  }
  DictRef dict_ref() const {
    DictRef D;
    D.words = dict_words; D.wmax = dict_wmax; D.nt = dict_nt; D.ntab = dict_ntab;
    D.codes = dcodes.as<uint64_t>();
    D.rtype = dict_typed ? drtype.as<uint8_t>() : nullptr;
    D.rwords = dict_typed ? drwords.as<uint64_t>() : nullptr;
    D.doff = doff.as<int32_t>();
    D.dval = dval.as<double>();
    D.scan_new = scan_new;
    D.hb = dict_hb;
    D.utd = (dict_typed && dutd.p) ? dutd.as<double>() : nullptr;
    D.uti = (dict_typed && duti.p) ? duti.as<int32_t>() : nullptr;
    return D;
  }
};

int g_row_types = 1;  // use the second-level (row type) coding when a matrix allows it

int g_index16 = 1;  // use 16-bit relative column indices when a matrix allows it
int g_nontemporal = 1;  // stream large matrices with non-temporal loads

int g_default_layout = AMG_HIP_LAYOUT_AUTO;

// Device copies drop entries that are exactly 0.0 (the Galerkin product keeps
// them structurally, SURVEY F5: 22 % of level 1).  x + 0*u == x for every finite
// u, so results are bit-identical; the host hierarchy (getters) keeps them.
Sparse without_exact_zeros(const Sparse& M) {
  Sparse R;
  R.n_outer = M.n_outer;
  R.n_inner = M.n_inner;
  R.ptr.assign(M.n_outer + 1, 0);
  R.idx.reserve(M.idx.size());
  R.val.reserve(M.val.size());
  for (int64_t o = 0; o < M.n_outer; ++o) {
    for (int32_t p = M.ptr[o]; p < M.ptr[o + 1]; ++p)
      if (M.val[p] != 0.0) {
        R.idx.push_back(M.idx[p]);
        R.val.push_back(M.val[p]);
      }
    R.ptr[o + 1] = (int32_t)R.idx.size();
  }
  return R;
}

hipError_t upload_mat(const Sparse& M, int layout, DevMat* D, int64_t diag_shift, bool allow16);

// K-Patch table of a dictionary-coded, row-typed matrix: finds the pitch m of the band (every
// column offset must be dj * m + di with dj, di in {-1, 0, 1}: the 5-point level and the
// 9-point Galerkin levels of a 2-D grid) and expands type -> code word -> pairs into
// {off-diagonal value, diagonal value, value, LDS offset} per (type, slot).
bool build_patch_table(const DictMat& T, int64_t n, int64_t* m_out, int* un_out, int* ntypes_out,
                       std::vector<double>* tab) {
  if (T.rwords.empty() || T.max_width > 9 || T.doff.empty()) return false;
  int64_t omax = 0;
  for (int32_t o : T.doff) omax = std::max<int64_t>(omax, o < 0 ? -(int64_t)o : o);
  int ntypes = 0;
  for (int t = 0; t < 255; ++t) {  // used types are numbered from 0; unused words are all 0xFF
    bool used = false;
    for (int k = 0; k < T.words; ++k) used = used || T.rwords[(size_t)t * T.words + k] != ~(uint64_t)0;
    if (used) ntypes = t + 1;
  }
  const int un = patch_un(T.max_width);
  if (ntypes < 1 || (ntypes + 1) * un > patch_max_entries()) return false;
  const int pitch = patch_lds_pitch();
  for (int64_t m : {omax, omax - 1}) {
    if (!patch_geometry_ok(n, m)) continue;
    bool ok = true;
    std::vector<double> out((size_t)ntypes * un * 4, 0.0);
    for (int t = 0; t < ntypes && ok; ++t)
      for (int e = 0; e < un; ++e) {
        double* q = &out[((size_t)t * un + e) * 4];
        const int code = e < 8 * T.words ? (int)((T.rwords[(size_t)t * T.words + e / 8] >> (8 * (e % 8))) & 0xFF) : 0xFF;
        if (code == 0xFF) { q[3] = -1.0e9; continue; }
        if (code >= (int)T.doff.size()) { ok = false; break; }
        const int64_t o = T.doff[code];
        const double v = T.dval[code];
        int64_t dj = 0;
        if (o > m / 2) dj = 1;
        else if (o < -(m / 2)) dj = -1;
        const int64_t di = o - dj * m;
        if (di < -1 || di > 1) { ok = false; break; }
        q[0] = o == 0 ? 0.0 : v;
        q[1] = o == 0 ? v : 0.0;
        q[2] = v;
        q[3] = (double)(dj * pitch + di);
      }
    if (!ok) continue;
    *m_out = m;
    *un_out = un;
    *ntypes_out = ntypes;
    tab->swap(out);
    return true;
  }
  return false;
}

// Common tail of the dictionary upload (host encoder: upload_mat; device encoder:
// device_dict_encode): the tables, the layout flags, the K-GS-scan distances and the K-Patch
// tables.  D->dict_typed and the per-row arrays (drtype or dcodes) are set by the caller;
// T needs words, max_width, doff, dval and, when typed, rwords.
hipError_t finish_dict(const DictMat& T, int64_t n, int64_t diag_shift, DevMat* D) {
  hipError_t e;
  D->dict = true;
  D->sell = false;
  D->dict_words = T.words;
  D->dict_wmax = T.max_width;
  D->dict_ntab = (int)T.doff.size();
  D->dict_shift = diag_shift;
  D->dict_hb = 0;
  for (int32_t o : T.doff) D->dict_hb = std::max<int>(D->dict_hb, o < 0 ? -o : o);
  // one sweep streams codes + f + out and gathers x: non-temporal stream when
  // that is well beyond the 256 MiB Infinity Cache
  const double stream_bytes = (double)n * ((D->dict_typed ? 1.0 : 8.0 * T.words) + 24.0);
  D->dict_nt = (g_nontemporal && stream_bytes > 192.0e6) ? 1 : 0;
  if (D->dict_typed)
    if ((e = upload(D->drwords, T.rwords.data(), T.rwords.size())) != hipSuccess) return e;
  if ((e = upload(D->doff, T.doff.data(), T.doff.size())) != hipSuccess) return e;
  if ((e = upload(D->dval, T.dval.data(), T.dval.size())) != hipSuccess) return e;
  if (D->dict_typed && diag_shift == 0 && T.rwords.size() >= (size_t)256 * T.words && T.words <= 2) {
    // The pairs of every row type laid out per slot, and whether its columns form the 7-point
    // pattern {-M, -m, -1, 0, 1, m, M} or the 15-point pattern {-M, -m, 0, m, M} x {-1, 0, 1} with
    // even m < M (kernels.hip: dict_rows_stencil): same values, same slot order as the LDS tables.
    std::vector<double> ud((size_t)256 * 33, 0.0);
    std::vector<int32_t> ui((size_t)256 * 18, 0);
    bool any = false;
    for (int t = 0; t < 255; ++t) {
      double diag = 0.0;
      int32_t mask = 0;
      int cnt = 0;
      int64_t o[16];
      bool dense = true;  // the slots in use are 0 .. cnt-1
      for (int sl = 0; sl < 8 * T.words; ++sl) {
        const int code = (int)((T.rwords[(size_t)t * T.words + sl / 8] >> (8 * (sl % 8))) & 0xFF);
        if (code == 0xFF || code >= (int)T.doff.size()) continue;
        const int32_t off = T.doff[(size_t)code];
        const double v = T.dval[(size_t)code];
        dense = dense && sl == cnt;
        o[cnt++] = off;
        ui[(size_t)t * 18 + sl] = off;
        ud[(size_t)t * 33 + 16 + sl] = v;
        ud[(size_t)t * 33 + sl] = off == 0 ? 0.0 : v;
        if (off == 0) diag = diag + v;
        mask |= (int32_t)1 << sl;
      }
      ud[(size_t)t * 33 + 32] = diag;
      ui[(size_t)t * 18 + 16] = mask;
      int pat = 0;
      if (dense && cnt == 7) {
        const int64_t m = o[5], M = o[6];
        if (o[0] == -M && o[1] == -m && o[2] == -1 && o[3] == 0 && o[4] == 1 && m > 1 && M > m && m % 2 == 0 &&
            M % 2 == 0)
          pat = 7;
      } else if (dense && cnt == 15) {
        const int64_t m = o[10], M = o[13];
        bool okp = m > 2 && M > m + 2 && m % 2 == 0 && M % 2 == 0;
        const int64_t c[5] = {-M, -m, 0, m, M};
        for (int k = 0; k < 5 && okp; ++k)
          okp = o[3 * k] == c[k] - 1 && o[3 * k + 1] == c[k] && o[3 * k + 2] == c[k] + 1;
        if (okp) pat = 15;
      }
      ui[(size_t)t * 18 + 17] = pat;
      any = any || pat != 0;
    }
    if (any) {
      if ((e = upload(D->dutd, ud.data(), ud.size())) != hipSuccess) return e;
      if ((e = upload(D->duti, ui.data(), ui.size())) != hipSuccess) return e;
    }
  }
  D->scan_gap = D->scan_far = 0;
  if (diag_shift == 0) {
    int64_t gap = INT64_MAX, far = 1;
    for (int32_t o : T.doff) {
      const int64_t a = o < 0 ? -(int64_t)o : o;
      if (a >= 2) gap = std::min(gap, a);
      far = std::max(far, a);
    }
    D->scan_gap = gap == INT64_MAX ? (int64_t)1 << 20 : gap;
    D->scan_far = far;
    D->scan_new = 99;
    if (!T.rwords.empty()) {  // per row type: entries below -1 / above +1
      int mx = 0;
      for (int t = 0; t < 255; ++t) {
        int lo = 0, hi = 0;
        for (int e = 0; e < 8 * T.words; ++e) {
          const int code = (int)((T.rwords[(size_t)t * T.words + e / 8] >> (8 * (e % 8))) & 0xFF);
          if (code == 0xFF || code >= (int)T.doff.size()) continue;
          if (T.doff[code] < -1) ++lo;
          if (T.doff[code] > 1) ++hi;
        }
        mx = std::max(mx, std::max(lo, hi));
      }
      D->scan_new = mx;
    }
  }
  D->march_ntypes = 0;
  if (D->dict_typed && diag_shift == 0 && T.rwords.size() >= (size_t)256 * T.words && T.words <= 2) {
    // K-March table: find the interior 7-point type, then lay every type out by pattern position
    int64_t pm = 0, pM = 0;
    int tint = -1;
    std::vector<std::vector<std::pair<int64_t, double>>> rows(255);
    int last = -1;
    for (int t = 0; t < 255; ++t) {
      for (int sl = 0; sl < 8 * T.words; ++sl) {
        const int code = (int)((T.rwords[(size_t)t * T.words + sl / 8] >> (8 * (sl % 8))) & 0xFF);
        if (code == 0xFF || code >= (int)T.doff.size()) continue;
        rows[(size_t)t].push_back({(int64_t)T.doff[(size_t)code], T.dval[(size_t)code]});
      }
      const auto& r = rows[(size_t)t];
      if (!r.empty()) last = t;
      if (tint < 0 && r.size() == 7 && r[2].first == -1 && r[3].first == 0 && r[4].first == 1 &&
          r[5].first > 1 && r[6].first > r[5].first && r[1].first == -r[5].first && r[0].first == -r[6].first &&
          r[6].first % r[5].first == 0) {
        tint = t;
        pm = r[5].first;
        pM = r[6].first;
      }
    }
    if (tint >= 0 && last < 64 && pM < ((int64_t)1 << 30) && n % pM == 0) {
      const int64_t P[6] = {-pM, -pm, -1, 1, pm, pM};
      std::vector<double> wt((size_t)(last + 1) * 8, 0.0);
      bool ok = true;
      for (int t = 0; t <= last && ok; ++t) {
        double diag = 0.0;
        for (const auto& e : rows[(size_t)t]) {
          if (e.first == 0) {
            diag = diag + e.second;
            continue;
          }
          int at = -1;
          for (int u = 0; u < 6; ++u)
            if (P[u] == e.first) at = u;
          if (at < 0) { ok = false; break; }
          wt[(size_t)t * 8 + at] = e.second;
        }
        wt[(size_t)t * 8 + 6] = diag;
      }
      if (ok) {  // the offsets alone do not make a box: no row may couple across a line or plane edge
        MarchForbid F;
        F.ntypes = last + 1;
        for (int t = 0; t <= last; ++t)
          for (const auto& e : rows[(size_t)t])
            F.bits[t] |= (uint8_t)((e.first == -1 ? 1 : 0) | (e.first == 1 ? 2 : 0) | (e.first == -pm ? 4 : 0) |
                                   (e.first == pm ? 8 : 0));
        DevMem dbad;
        int32_t bad = 0;
        if ((e = dbad.alloc(sizeof(int32_t))) != hipSuccess) return e;
        if ((e = hipMemset(dbad.p, 0, sizeof(int32_t))) != hipSuccess) return e;
        if ((e = launch_march_box_check(n, (int)pm, (int)(pM / pm), F, D->drtype.as<uint8_t>(),
                                        dbad.as<int32_t>(), nullptr)) != hipSuccess)
          return e;
        if ((e = hipMemcpy(&bad, dbad.p, sizeof(int32_t), hipMemcpyDeviceToHost)) != hipSuccess) return e;
        ok = bad == 0;
      }
      if (ok) {
        if ((e = upload(D->dmarch, wt.data(), wt.size())) != hipSuccess) return e;
        D->march_m = (int)pm;
        D->march_M = (int)pM;
        D->march_ntypes = last + 1;
        D->march_tint = tint;
        for (int u = 0; u < 6; ++u) D->march_wint[u] = wt[(size_t)tint * 8 + u];
        D->march_dint = wt[(size_t)tint * 8 + 6];
      }
    }
  }
  D->patch = false;
  if (D->dict_typed && diag_shift == 0) {
    std::vector<double> tab;
    if (build_patch_table(T, n, &D->patch_m, &D->patch_un, &D->patch_ntypes, &tab)) {
      if ((e = upload(D->patch_tab, tab.data(), tab.size())) != hipSuccess) return e;
      // per-type 3 x 3 slot form for the wave-uniform path (+ the all-absent type `ntypes`):
      // slot = (dj + 1) * 3 + (di + 1) = ascending column offset
      const int un = D->patch_un, nty = D->patch_ntypes, pitch = patch_lds_pitch();
      std::vector<double> ud((size_t)(nty + 1) * 19, 0.0);
      std::vector<int32_t> ui((size_t)(nty + 1) * 2, 0);
      for (int t = 0; t < nty; ++t) {
        double diag = 0.0;
        uint32_t rm = 0;
        for (int k = 0; k < un; ++k) {
          const double* q = &tab[((size_t)t * un + k) * 4];
          if (!(q[3] > -1.0e8)) continue;
          const int lo = (int)q[3];
          const int dj = lo > pitch / 2 ? 1 : (lo < -pitch / 2 ? -1 : 0), di = lo - dj * pitch;
          const int slot = (dj + 1) * 3 + (di + 1);
          ud[(size_t)t * 19 + slot] = q[0];
          ud[(size_t)t * 19 + 9 + slot] = q[2];
          diag += q[1];  // dict_rows' order: +0.0 except the diagonal slot
          rm |= 1u << slot;
        }
        ud[(size_t)t * 19 + 18] = diag;
        ui[(size_t)t * 2] = (int32_t)rm;
        ui[(size_t)t * 2 + 1] = (rm & 0x145u) ? 1 : 0;  // corner slots 0, 2, 6, 8
      }
      if ((e = upload(D->patch_utabd, ud.data(), ud.size())) != hipSuccess) return e;
      if ((e = upload(D->patch_utabi, ui.data(), ui.size())) != hipSuccess) return e;
      // which patches consist of one row type only (the interior of the level)
      int64_t tiles = 0;
      for (int rings = 2; rings <= 3; ++rings) {  // (3 last: `tiles` below counts the 42-line tiles)
        DevMem& F = rings == 2 ? D->patch_flags2 : D->patch_flags;
        DevMem& CT = rings == 2 ? D->patch_ctype2 : D->patch_ctype;
        if ((e = launch_patch_tile_flags(n, D->patch_m, rings, nullptr, nty, nullptr, &tiles, nullptr)) != hipSuccess) return e;
        // whole 32-bit words, zero-filled: the kernels read the word that holds a tile's flag
        if ((e = F.alloc(((size_t)tiles + 3) & ~(size_t)3)) != hipSuccess) return e;
        if ((e = hipMemset(F.p, 0, F.bytes)) != hipSuccess) return e;
        if ((e = alloc_patch_ctype(CT, tiles, rings)) != hipSuccess) return e;
        if ((e = launch_patch_tile_flags(n, D->patch_m, rings, D->drtype.as<uint8_t>(), nty, F.as<uint8_t>(),
                                         nullptr, nullptr, CT.as<uint8_t>())) != hipSuccess) return e;
      }
      if (patch_un(un) == 5) {  // the seam launch's tiles (the kernel kind it is instantiated for)
        int64_t t5 = 0;
        if ((e = launch_patch_seam_flags(n, D->patch_m, nullptr, nty, nullptr, &t5, nullptr)) == hipSuccess) {
          if ((e = D->patch_flags5.alloc(((size_t)t5 + 3) & ~(size_t)3)) != hipSuccess) return e;
          if ((e = hipMemset(D->patch_flags5.p, 0, D->patch_flags5.bytes)) != hipSuccess) return e;
          if ((e = alloc_patch_ctype(D->patch_ctype5, t5, 5)) != hipSuccess) return e;
          if ((e = launch_patch_seam_flags(n, D->patch_m, D->drtype.as<uint8_t>(), nty, D->patch_flags5.as<uint8_t>(),
                                           nullptr, nullptr, D->patch_ctype5.as<uint8_t>())) != hipSuccess) return e;
        }  // (a level too large for the seam frame's index range keeps the two launches: no flags, patch_seam_ok)
      }
      if ((e = hipDeviceSynchronize()) != hipSuccess) return e;
      // the interior row type = the type most tiles consist of; its slots choose the kernel kind
      {
        std::vector<uint8_t> fl((size_t)tiles);
        if ((e = hipMemcpy(fl.data(), D->patch_flags.p, fl.size(), hipMemcpyDeviceToHost)) != hipSuccess) return e;
        std::vector<int64_t> cnt(256, 0);
        for (uint8_t f : fl) ++cnt[f];
        int best = -1;
        for (int t = 0; t < nty; ++t)
          if (cnt[t] > 0 && (best < 0 || cnt[t] > cnt[best])) best = t;
        D->patch_umask = best >= 0 ? ui[(size_t)best * 2] : patch_default_umask(patch_un(un));
      }
      D->patch = true;
    }
  }
  return hipSuccess;
}

hipError_t upload_mat_pruned(const Sparse& M, int layout, bool prune, DevMat* D,
                             int64_t diag_shift = 0) {
  bool any = false;
  if (prune)
    for (double v : M.val)
      if (v == 0.0) { any = true; break; }
  if (!any) return upload_mat(M, layout, D, diag_shift, true);
  return upload_mat(without_exact_zeros(M), layout, D, diag_shift, true);
}

// layout: AMG_HIP_LAYOUT_*; AUTO takes SELL-64 unless padding exceeds 25 %.
// diag_shift: column of row i's diagonal is i + diag_shift (0 except for the
// halo-extended local blocks of the multi-GPU driver); only used to decide
// whether 16-bit relative column indices fit.
hipError_t upload_mat(const Sparse& M, int layout, DevMat* D, int64_t diag_shift, bool allow16);
hipError_t upload_mat(const Sparse& M, int layout, DevMat* D) {
  return upload_mat(M, layout, D, 0, true);
}
hipError_t upload_mat(const Sparse& M, int layout, DevMat* D, int64_t diag_shift, bool allow16) {
  D->n_rows = M.n_outer;
  D->nnz = M.nnz();
  D->dict = false;
  if ((layout == AMG_HIP_LAYOUT_AUTO || layout == AMG_HIP_LAYOUT_DICT) && allow16 &&
      M.n_outer < ((int64_t)1 << 31) - 512) {
    DictMat T;
    if (to_dict(M, diag_shift, &T)) {
      hipError_t e;
      D->dict_typed = g_row_types != 0 && !T.rtype.empty();
      if (D->dict_typed) {  // the kernels then never touch the per-row code words
        if ((e = upload(D->drtype, T.rtype.data(), T.rtype.size())) != hipSuccess) return e;
      } else {
        if ((e = upload(D->dcodes, T.codes.data(), T.codes.size())) != hipSuccess) return e;
      }
      return finish_dict(T, M.n_outer, diag_shift, D);
    }
    if (layout == AMG_HIP_LAYOUT_DICT) layout = AMG_HIP_LAYOUT_SELL;
  }
  if (layout == AMG_HIP_LAYOUT_DICT) layout = AMG_HIP_LAYOUT_SELL;
  bool sell = layout == AMG_HIP_LAYOUT_SELL;
  Sell64 S;
  if (layout != AMG_HIP_LAYOUT_CSR && M.n_outer < ((int64_t)1 << 31) - 512) {
    to_sell64(M, &S);
    if (layout == AMG_HIP_LAYOUT_AUTO) sell = (double)S.slots() <= 1.25 * (double)M.nnz() + 4096.0;
  } else {
    sell = false;
  }
  D->sell = sell;
  if (!sell) return upload_csr(M, &D->csr);
  D->max_width = S.max_width;
  D->slots = S.slots();
  hipError_t e;
  if ((e = upload(D->soff, S.soff.data(), S.soff.size())) != hipSuccess) return e;
  // 16-bit relative indices when every entry is within +-32767 of its row's diagonal
  bool fits = allow16 && g_index16 != 0;
  std::vector<int16_t> c16;
  if (fits) {
    c16.assign(S.col.size(), (int16_t)-32768);
    const int64_t np = (int64_t)S.soff.size() - 1;
    for (int64_t p = 0; p < np && fits; ++p) {
      const int64_t w = (S.soff[p + 1] - S.soff[p]) / 64;
      for (int64_t j = 0; j < w && fits; ++j)
        for (int64_t l = 0; l < 64; ++l) {
          const int64_t at = S.soff[p] + j * 64 + l;
          const int32_t c = S.col[at];
          if (c < 0) continue;
          const int64_t d = (int64_t)c - (p * 64 + l + diag_shift);
          if (d < -32767 || d > 32767) { fits = false; break; }
          c16[at] = (int16_t)d;
        }
    }
  }
  // non-temporal matrix stream for matrices well beyond the 256 MiB Infinity Cache
  const double stream_bytes = (double)S.slots() * (fits ? 10.0 : 12.0);
  D->idx16 = (fits ? 1 : 0) | ((g_nontemporal && stream_bytes > 192.0e6) ? 2 : 0);
  if (fits) {
    if ((e = upload(D->scol, c16.data(), c16.size())) != hipSuccess) return e;
  } else {
    if ((e = upload(D->scol, S.col.data(), S.col.size())) != hipSuccess) return e;
  }
  return upload(D->sval, S.val.data(), S.val.size());
}

hipError_t launch_mat(int mode, const DevMat& A, const double* x, const double* f, double* out,
                      double omega, hipStream_t st, int64_t diag_shift = 0) {
  if (A.dict) {
    if (diag_shift != A.dict_shift) return hipErrorInvalidValue;  // offsets are baked in
    return launch_dict(mode, A.n_rows, A.dict_ref(), x, f, out, omega, diag_shift, st);
  }
  if (A.sell)
    return launch_sell(mode, A.n_rows, A.idx16, A.soff.as<int64_t>(), A.scol.p,
                       A.sval.as<double>(), x, f, out, omega, diag_shift, st);
  const DevCsr& C = A.csr;
  return launch_csr(mode, C.n_rows, C.nnz, C.max_block_nnz, C.max_row_nnz, C.rowptr(), C.col(),
                    C.v(), x, f, out, omega, diag_shift, st);
}

// one Chebyshev step (kernels.hpp: CSR_CHEB) on a level matrix in its device layout
hipError_t launch_mat_cheb(const DevMat& A, const double* x, const double* f, double* out, const ChebStep& c,
                           hipStream_t st) {
  if (A.dict) {
    if (A.dict_shift != 0) return hipErrorInvalidValue;
    return launch_dict_cheb(A.n_rows, A.dict_ref(), x, f, out, c, st);
  }
  if (A.sell)
    return launch_sell_cheb(A.n_rows, A.idx16, A.soff.as<int64_t>(), A.scol.p, A.sval.as<double>(), x, f, out, c,
                            st);
  const DevCsr& C = A.csr;
  return launch_csr_cheb(C.n_rows, C.nnz, C.max_block_nnz, C.max_row_nnz, C.rowptr(), C.col(), C.v(), x, f, out,
                         c, st);
}

// Chebyshev smoother: "" when the options are valid
std::string cheb_options_error(int32_t degree, double lower, double upper) {
  if (degree < 1) return "`cheb_degree` must be at least 1, got " + std::to_string(degree);
  if (!(lower > 0.0)) return "`cheb_lower` must be > 0, got " + std::to_string(lower);
  if (!(lower < upper))
    return "`cheb_lower` must be < `cheb_upper`, got " + std::to_string(lower) + " and " + std::to_string(upper);
  return "";
}
// Gershgorin bound of D^-1 A from CSR rows: max_i (sum_j |a_ij|) / |a_ii|, each row summed in
// ascending column order (the device kernel's order: launch_gershgorin).  *zero_row: first row
// whose diagonal is zero or absent, else -1.
double gershgorin_host(const Sparse& Ar, int64_t* zero_row) {
  double G = 0.0;
  *zero_row = -1;
  for (int64_t i = 0; i < Ar.n_outer; ++i) {
    double sum = 0.0, dg = 0.0;
    for (int32_t p = Ar.ptr[i]; p < Ar.ptr[i + 1]; ++p) {
      sum += std::fabs(Ar.val[p]);
      if (Ar.idx[p] == i) dg = Ar.val[p];
    }
    if (dg == 0.0) {
      if (*zero_row < 0) *zero_row = i;
      continue;
    }
    const double g = sum / std::fabs(dg);
    if (g > G) G = g;
  }
  return G;
}
std::string cheb_zero_diag(int l, int64_t row) {
  return "Chebyshev smoother: level " + std::to_string(l) + " row " + std::to_string(row) +
         " has a zero diagonal (D^-1 A does not exist)";
}
// the step coefficients of one application, in double, in this order (include/amg_hip.h: cheb_lower)
void cheb_coefs(double lo, double hi, int k, std::vector<double>* alpha, std::vector<double>* beta) {
  const double theta = (hi + lo) / 2, delta = (hi - lo) / 2;
  const double sigma = theta / delta;
  double rho = 1.0 / sigma;
  alpha->assign((size_t)k, 0.0);
  beta->assign((size_t)k, 0.0);
  (*beta)[0] = 1.0 / theta;
  for (int i = 1; i < k; ++i) {
    const double rn = 1.0 / (2.0 * sigma - rho);
    (*alpha)[(size_t)i] = rn * rho;
    (*beta)[(size_t)i] = 2.0 * rn / delta;
    rho = rn;
  }
}

// ---- line smoother (AMG_HIP_SM_LINE_JACOBI; kernels.hip: K-Line) ----
std::string line_options_error(double omega) {
  if (!(omega > 0.0 && omega < 2.0))
    return "line smoother: `omega` must lie in (0, 2), got " + std::to_string(omega);
  return "";
}
// dir: the direction of AMG_HIP_SM_LINE_ALT whose elimination failed ("x", "y", "z"), else null
std::string line_bad_pivot(int l, int64_t row, const char* dir = nullptr) {
  return "line smoother: level " + std::to_string(l) + (dir ? std::string(" direction ") + dir : std::string()) +
         " row " + std::to_string(row) +
         " has a zero or non-finite pivot in the elimination of its line (the smoother needs a diagonally "
         "dominant operator)";
}
struct LineOnDev {  // factors of T (n doubles each) and the scratch vector y
  int64_t n = 0, s = 0;
  int64_t m = 0;  // LineRef::m
  int cyc = 0;    // LineRef::cyc
  DevMem dl, ip, cp, v, w, y;
  LineRef ref() const {
    LineRef R;
    R.n = n;
    R.s = s;
    R.m = m;
    R.cyc = cyc;
    R.dl = dl.as<double>();
    R.ip = ip.as<double>();
    R.cp = cp.as<double>();
    R.v = v.as<double>();
    R.w = w.as<double>();
    return R;
  }
  // rows on a separator position (p % LINE_SEG == LINE_SEG - 1 on their chain)
  int64_t separators() const {
    int64_t k = 0;
    if (s < 1 || s > n) return 0;  // line_setup_dev clamps the stride to n
    for (int64_t p = LINE_SEG - 1; p * s < n; p += LINE_SEG) k += std::min<int64_t>(s, n - p * s);
    return k;
  }
  // bytes one u += omega T^-1 r has to move: interior rows r, dl, ip, cp in and y out, then y, v, w, u
  // in and u out (80 B); separator rows r, dl, w, v, ip, cp, both neighbours' y in and y out, then
  // y, u in and u out (96 B)
  double solve_bytes() const {
    const int64_t sep = separators();
    return 80.0 * (double)(n - sep) + 96.0 * (double)sep;
  }
};
// stride (0: the automatic rule, on the device) and factors of one level from its device CSR rows
amg_hip_status line_setup_dev(int l, int64_t n, const int32_t* rowptr, const int32_t* col, const double* val,
                              int64_t stride, LineOnDev* out, int64_t m = 0, const char* dir = nullptr,
                              int cyc = 0) {
  LineOnDev& D = *out;
  D.n = n;
  D.m = m;
  D.cyc = cyc;
  for (DevMem* m : {&D.dl, &D.ip, &D.cp, &D.v, &D.w, &D.y}) HIP_TRY(m->alloc(sizeof(double) * (size_t)n));
  DevMem flag;
  HIP_TRY(flag.alloc(sizeof(uint64_t) * 2));
  uint64_t h[2];
  if (stride < 1) {
    HIP_TRY(launch_line_stride(n, rowptr, col, val, D.y.as<double>(), flag.as<uint64_t>(), nullptr));
    HIP_TRY(hipMemcpy(h, flag.p, sizeof(h), hipMemcpyDeviceToHost));
    stride = (int64_t)h[1];
  }
  // s >= n: every row is its own chain, whatever s is; n stands for all of them, so that the index
  // arithmetic of the kernels (positions times s) stays far from overflow
  D.s = std::min<int64_t>(stride, n);
  HIP_TRY(launch_line_setup(D.ref(), rowptr, col, val, flag.as<uint64_t>(), nullptr));
  HIP_TRY(hipMemcpy(h, flag.p, sizeof(h), hipMemcpyDeviceToHost));
  if (h[0] != ~(uint64_t)0) return fail(AMG_HIP_EINVAL, line_bad_pivot(l, (int64_t)h[0], dir));
  return AMG_HIP_OK;
}

// ---- alternating-direction line smoother (AMG_HIP_SM_LINE_ALT; kernels.hip: K-LineX, K-Line) ----
// The directions of a level: its axes of length >= 2 in the order x, y, z.  x runs as K-LineX, y and
// z as K-Line with the strides nx and nx ny (m = ny, nz: entries across a plane end stay out of T).
// A level without a direction (one row) is weighted Jacobi: K-Line with every row its own chain.
// Cyclic directions (opt.cyclic_lines: a periodic axis of length >= 3): the factors are those of T',
// and K-LineSeam corrects the residual between the residual and the solve (kernels.hpp: SeamRef).
const char* const ALT_AXIS[3] = {"x", "y", "z"};
const char* const ALT_NEEDS_GRID =
    "unknown smoother kind for this constructor: AMG_HIP_SM_LINE_ALT needs the level grids of amg_hip_create_tensor";
struct AltOnDev {
  int n_dir = 0;
  int axis[3] = {0, 0, 0};
  int64_t stride[3] = {0, 0, 0}, len[3] = {0, 0, 0};
  int64_t n = 0;
  DevMem xdl, xip, xcp;  // K-LineX factors (direction x)
  LineOnDev yz[2];       // K-Line factors of the directions y, z; yz[0] of the level without directions
  bool cyc[3] = {false, false, false};  // direction d is solved cyclically
  DevMem seam_p[3], seam_coef[3];       // SeamRef::p, ::coef of the cyclic directions
  // cyclic: the periodic axes whose lines are solved cyclically where the level has 3 points or more
  void set_grid(int64_t rows, const int64_t dims[3], uint32_t cyclic = 0) {
    n = rows;
    n_dir = 0;
    int64_t st = 1;
    for (int a = 0; a < 3; ++a) {
      if (dims[a] >= 2) {
        axis[n_dir] = a;
        stride[n_dir] = st;
        len[n_dir] = dims[a];
        cyc[n_dir] = ((cyclic >> a) & 1u) && dims[a] >= 3;
        ++n_dir;
      }
      st *= dims[a];
    }
  }
  LineXRef xref() const {
    LineXRef R;
    R.n = n;
    R.nx = len[0];
    R.dl = xdl.as<double>();
    R.ip = xip.as<double>();
    R.cp = xcp.as<double>();
    return R;
  }
  int32_t cyclic_mask() const {
    int32_t mask = 0;
    for (int d = 0; d < n_dir; ++d)
      if (cyc[d]) mask |= 1 << axis[d];
    return mask;
  }
  SeamRef seam(int d) const {
    SeamRef S;
    S.n = n;
    S.s = stride[d];
    S.m = len[d];
    S.p = seam_p[d].as<double>();
    S.coef = seam_coef[d].as<double>();
    return S;
  }
  // What sub-sweep d runs (d = 0 on a level without directions): K-LineSeam first where cyclic(d), then
  // K-LineX where along_x(d), else K-Line with yz[yz_of(d)]
  bool cyclic(int d) const { return n_dir > 0 && cyc[d]; }
  bool along_x(int d) const { return n_dir > 0 && axis[d] == 0; }
  int yz_of(int d) const { return n_dir == 0 || axis[d] == 0 ? 0 : axis[d] - 1; }
  // K-LineSeam of a cyclic direction: p and r in (16 B per row); den, gamma, beta in and the two ends
  // of r out (40 B per line)
  double seam_bytes(int d) const {
    return d < n_dir && cyc[d] ? 16.0 * (double)n + 40.0 * (double)(n / len[d]) : 0.0;
  }
  // bytes the solve of direction d (or of the level without directions, d = 0) has to move.  K-LineX:
  // r, dl, ip in and y out, then y, cp, u in and u out: 64 B per row
  double solve_bytes(int d) const {
    if (n_dir == 0) return yz[0].solve_bytes();
    return (axis[d] == 0 ? 64.0 * (double)n : yz[axis[d] - 1].solve_bytes()) + seam_bytes(d);
  }
};
std::string seam_bad_den(int l, int64_t row, const char* dir) {
  return "line smoother: level " + std::to_string(l) + " direction " + dir + " row " + std::to_string(row) +
         " starts a cyclic line whose Sherman-Morrison denominator is zero or not finite (the cyclic line "
         "operator is singular or far from diagonally dominant)";
}
// host_only: the pivot check of every direction on the host
amg_hip_status alt_setup_host(int l, const int32_t* rowptr, const int32_t* col, const double* val, AltOnDev* D) {
  if (D->n_dir == 0) {
    const int64_t bad = line_setup_host(D->n, D->n, rowptr, col, val);
    if (bad >= 0) return fail(AMG_HIP_EINVAL, line_bad_pivot(l, bad));
  }
  for (int d = 0; d < D->n_dir; ++d) {
    // a cyclic direction: the pivots of T', those of its transpose, then the denominators
    for (int cyc = D->cyc[d] ? 1 : 0; cyc <= (D->cyc[d] ? 2 : 0); ++cyc) {
      const int64_t bad = D->axis[d] == 0
                              ? linex_setup_host(D->n, D->len[d], rowptr, col, val, cyc)
                              : line_setup_host(D->n, D->stride[d], rowptr, col, val, D->len[d], cyc);
      if (bad >= 0) return fail(AMG_HIP_EINVAL, line_bad_pivot(l, bad, ALT_AXIS[D->axis[d]]));
    }
    if (D->cyc[d]) {
      const int64_t bad = seam_setup_host(D->n, D->stride[d], D->len[d], rowptr, col, val);
      if (bad >= 0) return fail(AMG_HIP_EINVAL, seam_bad_den(l, bad, ALT_AXIS[D->axis[d]]));
    }
  }
  return AMG_HIP_OK;
}
// factors of direction x into X (K-LineX set-up)
amg_hip_status altx_factor_dev(int l, const LineXRef& X, const int32_t* rowptr, const int32_t* col,
                               const double* val) {
  DevMem flag;
  HIP_TRY(flag.alloc(sizeof(uint64_t) * 2));
  uint64_t h[2];
  HIP_TRY(launch_linex_setup(X, rowptr, col, val, flag.as<uint64_t>(), nullptr));
  HIP_TRY(hipMemcpy(h, flag.p, sizeof(h), hipMemcpyDeviceToHost));
  if (h[0] != ~(uint64_t)0) return fail(AMG_HIP_EINVAL, line_bad_pivot(l, (int64_t)h[0], ALT_AXIS[0]));
  return AMG_HIP_OK;
}
// The cyclic direction d, after its factors of T': p = T'^-T v (kept) from the factors of T'^T on
// temporaries, q = T'^-1 u (a temporary) with the kept factors, then den, gamma, beta of every line.
// Both solves are the sub-sweep's own launchers on a zero vector with omega = 1.
amg_hip_status alt_seam_setup_dev(int l, int d, const int32_t* rowptr, const int32_t* col, const double* val,
                                  AltOnDev* D) {
  const int64_t n = D->n, s = D->stride[d], m = D->len[d];
  const int a = D->axis[d];
  DevMem u, v, q, flag;
  for (DevMem* x : {&u, &v, &q, &D->seam_p[d]}) HIP_TRY(x->alloc(sizeof(double) * (size_t)n));
  HIP_TRY(D->seam_coef[d].alloc(sizeof(double) * 3 * (size_t)(n / m)));
  HIP_TRY(flag.alloc(sizeof(uint64_t) * 2));
  HIP_TRY(launch_seam_rhs(n, s, m, rowptr, col, val, u.as<double>(), v.as<double>(), nullptr));
  HIP_TRY(hipMemsetAsync(q.p, 0, sizeof(double) * (size_t)n, nullptr));
  HIP_TRY(hipMemsetAsync(D->seam_p[d].p, 0, sizeof(double) * (size_t)n, nullptr));
  if (a == 0) {
    DevMem tdl, tip, tcp;
    for (DevMem* x : {&tdl, &tip, &tcp}) HIP_TRY(x->alloc(sizeof(double) * (size_t)n));
    LineXRef T = D->xref();
    T.dl = tdl.as<double>();
    T.ip = tip.as<double>();
    T.cp = tcp.as<double>();
    T.cyc = 2;
    const amg_hip_status r = altx_factor_dev(l, T, rowptr, col, val);
    if (r != AMG_HIP_OK) return r;
    HIP_TRY(launch_linex_solve(T, v.as<double>(), D->seam_p[d].as<double>(), 1.0, nullptr));
    HIP_TRY(launch_linex_solve(D->xref(), u.as<double>(), q.as<double>(), 1.0, nullptr));
    HIP_TRY(hipDeviceSynchronize());  // the temporaries go out of scope
  } else {
    LineOnDev T;
    const amg_hip_status r = line_setup_dev(l, n, rowptr, col, val, s, &T, m, ALT_AXIS[a], 2);
    if (r != AMG_HIP_OK) return r;
    HIP_TRY(launch_line_solve(T.ref(), v.as<double>(), T.y.as<double>(), D->seam_p[d].as<double>(), 1.0, nullptr));
    const LineOnDev& Y = D->yz[a - 1];
    HIP_TRY(launch_line_solve(Y.ref(), u.as<double>(), Y.y.as<double>(), q.as<double>(), 1.0, nullptr));
    HIP_TRY(hipDeviceSynchronize());
  }
  uint64_t h[2];
  HIP_TRY(launch_seam_coef(n, s, m, rowptr, col, val, q.as<double>(), D->seam_coef[d].as<double>(),
                           flag.as<uint64_t>(), nullptr));
  HIP_TRY(hipMemcpy(h, flag.p, sizeof(h), hipMemcpyDeviceToHost));
  if (h[0] != ~(uint64_t)0) return fail(AMG_HIP_EINVAL, seam_bad_den(l, (int64_t)h[0], ALT_AXIS[a]));
  return AMG_HIP_OK;
}
amg_hip_status alt_setup_dev(int l, const int32_t* rowptr, const int32_t* col, const double* val, AltOnDev* D) {
  const int64_t n = D->n;
  if (D->n_dir == 0) return line_setup_dev(l, n, rowptr, col, val, n, &D->yz[0]);
  for (int d = 0; d < D->n_dir; ++d) {
    const int a = D->axis[d];
    if (a > 0) {
      const amg_hip_status r = line_setup_dev(l, n, rowptr, col, val, D->stride[d], &D->yz[a - 1], D->len[d],
                                              ALT_AXIS[a], D->cyc[d] ? 1 : 0);
      if (r != AMG_HIP_OK) return r;
    } else {
      for (DevMem* m : {&D->xdl, &D->xip, &D->xcp}) HIP_TRY(m->alloc(sizeof(double) * (size_t)n));
      LineXRef X = D->xref();
      X.cyc = D->cyc[d] ? 1 : 0;
      const amg_hip_status r = altx_factor_dev(l, X, rowptr, col, val);
      if (r != AMG_HIP_OK) return r;
    }
    if (D->cyc[d]) {
      const amg_hip_status r = alt_seam_setup_dev(l, d, rowptr, col, val, D);
      if (r != AMG_HIP_OK) return r;
    }
  }
  return AMG_HIP_OK;
}

// ---- one line sub-sweep and one smoothing application, for the double, the block and the float cycle ----
// The launchers of one precision and pitch behind one signature.  kp = 0: plain double vectors (the
// single-vector kernels); kp >= 1: the n x kp panels of the block cycle (K-LineBlock).  Float vectors
// are always plain.
hipError_t line_seam_any(int kp, const SeamRef& S, double* r, hipStream_t st) {
  return kp ? launch_block_line_seam(kp, S, r, st) : launch_line_seam(S, r, st);
}
hipError_t line_seam_any(int, const SeamRefT<float>& S, float* r, hipStream_t st) {
  return launch_line_seam_f32(S, r, st);
}
hipError_t linex_solve_any(int kp, const LineXRef& X, double* r, double* u, double omega, hipStream_t st) {
  return kp ? launch_block_linex_solve(kp, X, r, u, omega, st) : launch_linex_solve(X, r, u, omega, st);
}
hipError_t linex_solve_any(int, const LineXRefT<float>& X, float* r, float* u, float omega, hipStream_t st) {
  return launch_linex_solve_f32(X, r, u, omega, st);
}
hipError_t line_solve_any(int kp, const LineRef& Y, const double* r, double* y, double* u, double omega,
                          hipStream_t st) {
  return kp ? launch_block_line_solve(kp, Y, r, y, u, omega, st) : launch_line_solve(Y, r, y, u, omega, st);
}
hipError_t line_solve_any(int, const LineRefT<float>& Y, const float* r, float* y, float* u, float omega,
                          hipStream_t st) {
  return launch_line_solve_f32(Y, r, y, u, omega, st);
}
// A sub-sweep after its residual r = f - A u: K-LineSeam on r where the direction is cyclic (S), then
// u += omega T^-1 r as K-LineX where the direction is the x axis (X), else as K-Line with Y and the
// scratch y.  X and S are null where the direction has none.
template <typename T>
hipError_t launch_line_dir(const LineRefT<T>& Y, const LineXRefT<T>* X, const SeamRefT<T>* S, int kp, T* r, T* y,
                           T* u, T omega, hipStream_t st) {
  hipError_t e;
  if (S && (e = line_seam_any(kp, *S, r, st)) != hipSuccess) return e;
  return X ? linex_solve_any(kp, *X, r, u, omega, st) : line_solve_any(kp, Y, r, y, u, omega, st);
}
// launch_line_dir for direction d of D (AltOnDev::cyclic).  y: the scratch panel of the block cycle;
// plain vectors (kp = 0) use the direction's own
hipError_t launch_alt_dir(const AltOnDev& D, int d, int kp, double* r, double* y, double* u, double omega,
                          hipStream_t st) {
  const SeamRef S = D.seam(d);
  const LineXRef X = D.xref();
  const LineOnDev& Y = D.yz[D.yz_of(d)];
  return launch_line_dir(Y.ref(), D.along_x(d) ? &X : nullptr, D.cyclic(d) ? &S : nullptr, kp, r,
                         kp ? y : Y.y.as<double>(), u, omega, st);
}
// One smoothing application of a line smoother: `iters` times its nd sub-sweeps, the directions
// ascending on the way down and descending on the way up (reverse).  sub(d) enqueues sub-sweep d.
template <typename F>
amg_hip_status line_subsweeps(int64_t iters, int nd, bool reverse, F&& sub) {
  for (int64_t it = 0; it < iters; ++it)
    for (int q = 0; q < nd; ++q) AMG_TRY(sub(reverse ? nd - 1 - q : q));
  return AMG_HIP_OK;
}
// sub-sweeps of one application: AMG_HIP_SM_LINE_ALT one per direction, AMG_HIP_SM_LINE_JACOBI one
int line_dirs(int32_t smoother, const AltOnDev& D) {
  return smoother == AMG_HIP_SM_LINE_ALT ? std::max(D.n_dir, 1) : 1;
}
// `passes` sweeps that ping-pong u -> tmp -> u ...: sweep(i, in, out) enqueues the i-th; after an odd
// count the result sits in tmp and copy_home() brings it to u (keeps a captured graph static)
template <typename T, typename Sweep, typename Home>
amg_hip_status ping_pong(int64_t passes, T* u, T* tmp, Sweep&& sweep, Home&& copy_home) {
  for (int64_t i = 0; i < passes; ++i) {
    AMG_TRY(sweep(i, u, tmp));
    std::swap(u, tmp);
  }
  return (passes & 1) ? copy_home() : AMG_HIP_OK;
}
// The Chebyshev smoother: `iters` applications of the degree-k polynomial on [lo, hi], each k steps from
// step 0, as one ping-pong.  step(alpha, beta, first, last, in, out) enqueues one step of an application.
template <typename T, typename Step, typename Home>
amg_hip_status cheb_steps(double lo, double hi, int iters, int k, T* u, T* tmp, Step&& step, Home&& copy_home) {
  std::vector<double> alpha, beta;
  cheb_coefs(lo, hi, k, &alpha, &beta);
  return ping_pong((int64_t)iters * k, u, tmp, [&](int64_t i, T* a, T* b) {
    const size_t j = (size_t)(i % k);
    return step(alpha[j], beta[j], j == 0, (int)j == k - 1, a, b);
  }, copy_home);
}
// sub-sweep of AMG_HIP_SM_LINE_JACOBI on plain vectors: u <- u + omega T^-1 (f - A u); r: n doubles of scratch
hipError_t launch_line_sweep(const DevMat& A, const LineOnDev& D, double* u, const double* f, double* r,
                             double omega, hipStream_t st) {
  hipError_t e = launch_mat(CSR_RESID, A, u, f, r, 1.0, st);
  if (e != hipSuccess) return e;
  return launch_line_dir<double>(D.ref(), nullptr, nullptr, 0, r, D.y.as<double>(), u, omega, st);
}
// sub-sweep d of AMG_HIP_SM_LINE_ALT: u <- u + omega T_a^-1 (f - A u)
hipError_t launch_alt_subsweep(const DevMat& A, const AltOnDev& D, int d, double* u, const double* f, double* r,
                               double omega, hipStream_t st) {
  hipError_t e = launch_mat(CSR_RESID, A, u, f, r, 1.0, st);
  if (e != hipSuccess) return e;
  return launch_alt_dir(D, d, 0, r, nullptr, u, omega, st);
}

struct SpikeOnDev {  // device copy of a SpikeFactor + scratch
  SpikeArgs a{};
  DevMem sf, sb, d, V, W, Vt, Wh, G, Z, T, H;
};
hipError_t upload_spike(const SpikeFactor& S, SpikeOnDev* D) {
  hipError_t e;
  if ((e = upload(D->sf, S.sched_f.data(), S.sched_f.size())) != hipSuccess) return e;
  if ((e = upload(D->sb, S.sched_b.data(), S.sched_b.size())) != hipSuccess) return e;
  if ((e = upload(D->d, S.d.data(), S.d.size())) != hipSuccess) return e;
  if ((e = upload(D->V, S.V.data(), S.V.size())) != hipSuccess) return e;
  if ((e = upload(D->W, S.W.data(), S.W.size())) != hipSuccess) return e;
  if ((e = upload(D->Vt, S.Vt.data(), S.Vt.size())) != hipSuccess) return e;
  if ((e = upload(D->Wh, S.Wh.data(), S.Wh.size())) != hipSuccess) return e;
  const size_t wq = S.w > 0 ? S.w : 1;
  if ((e = D->G.alloc(sizeof(double) * (size_t)S.n)) != hipSuccess) return e;
  if ((e = D->Z.alloc(sizeof(double) * (size_t)S.n)) != hipSuccess) return e;
  if ((e = D->T.alloc(sizeof(double) * (size_t)(S.P + 1) * wq)) != hipSuccess) return e;
  if ((e = D->H.alloc(sizeof(double) * (size_t)(S.P + 1) * wq)) != hipSuccess) return e;
  SpikeArgs& a = D->a;
  a.n = S.n; a.w = S.w; a.c = S.c; a.P = S.P; a.m = S.m; a.sched_stride = S.sched_stride;
  a.sched_f = D->sf.as<double>(); a.sched_b = D->sb.as<double>(); a.d = D->d.as<double>();
  a.V = D->V.as<double>(); a.W = D->W.as<double>(); a.Vt = D->Vt.as<double>();
  a.Wh = D->Wh.as<double>(); a.G = D->G.as<double>(); a.Z = D->Z.as<double>();
  a.T = D->T.as<double>(); a.H = D->H.as<double>();
  return hipSuccess;
}

// The factored coarsest operator on the device in one of three forms:
//   BAND  one-wave substitution, half-bandwidth <= 63, bit-exact against the oracle
//   SPIKE partitioned (parallel) form of the same factor, <= 63, agrees to ~1e-14
//   WIDE  blocked one-wave substitution for any half-bandwidth, bit-exact
enum CoarseKind { COARSE_BAND = 0, COARSE_SPIKE = 1, COARSE_WIDE = 2, COARSE_CHAIN = 3 };
int g_no_band_chain = 0;  // amg_hip_set_band_chain
struct CoarseOnDev {
  int kind = COARSE_BAND;
  int64_t n = 0, w = 0;
  int m = 0;
  DevMem sf, sb, d;                  // BAND / WIDE schedules
  std::unique_ptr<SpikeOnDev> spike;
  bool pin = false;                  // opt.singular: the factor is that of pinned_last(A), see launch_coarse
};
// level-0 rows from which the lexicographic smoothers take the line-scan form by default
constexpr int64_t GS_SCAN_MIN_ROWS = 65536;
// ... and the shortest chunk worth it.  A chunk of at most 64 rows is one wave's scan without a
// barrier (~0.3 us), a serial row of the exact kernel costs ~0.33 us: from two rows per chunk on the
// scan form wins (round 3: 4 -> 2; 4096^2 / 16 levels 217 -> 198 ms per cycle, 1024^2 / 12 levels
// 30.4 -> 26.1 ms, and a hierarchy without exact-kernel levels is set up on the device: 2.75 ->
// 0.48 s).  AMG_HIP_SCAN_MIN_GAP overrides.
static const int64_t GS_SCAN_MIN_GAP = [] {
  const char* e = std::getenv("AMG_HIP_SCAN_MIN_GAP");
  return e ? (int64_t)std::atoi(e) : (int64_t)2;
}();
// serial substitution costs ~44 ns per row and pass; from this size on the partitioned
// solve is the default (opt.exact_coarse_solve keeps the bit-exact one)
constexpr int64_t COARSE_SPIKE_MIN_ROWS = 4096;
// multicolour GS: levels of at most this many rows run a whole symmetric pass as ONE launch
// (one workgroup, barriers between the colours) instead of one launch per colour and direction
// Multicolour levels of at most this many rows run the whole symmetric pass in ONE launch (one
// workgroup, a barrier between colours) instead of one launch per colour and direction; larger
// levels lose more to the single CU than the launches cost.  AMG_HIP_MC_ONE_LAUNCH_ROWS overrides
// (tuning / A-B; same bits).
int64_t mc_one_launch_max_rows() {
  static const int64_t v = [] {
    const char* e = std::getenv("AMG_HIP_MC_ONE_LAUNCH_ROWS");
    return e ? std::atoll(e) : (int64_t)8192;
  }();
  return v;
}
// Singular solvers (opt.singular: A semidefinite, the constants its null space): A with its last row
// and column replaced by those of the identity.  With the last entry of the right-hand side zeroed,
// every kind of the banded solve then returns x[n-1] = +0.0 and x[0 : n-1] = the solution of the
// leading principal block, which is SPD.
Sparse pinned_last(const Sparse& A) {
  const int32_t last = (int32_t)A.n_outer - 1;
  Sparse B;
  B.n_outer = A.n_outer;
  B.n_inner = A.n_inner;
  B.ptr.assign(1, 0);
  B.ptr.reserve(A.ptr.size());
  B.idx.reserve(A.idx.size());
  B.val.reserve(A.val.size());
  for (int32_t c = 0; c <= last; ++c) {
    if (c == last) {
      B.idx.push_back(last);
      B.val.push_back(1.0);
    } else {
      for (int32_t p = A.ptr[(size_t)c], e = A.ptr[(size_t)c + 1]; p < e; ++p)
        if (A.idx[(size_t)p] != last) {
          B.idx.push_back(A.idx[(size_t)p]);
          B.val.push_back(A.val[(size_t)p]);
        }
    }
    B.ptr.push_back((int32_t)B.idx.size());
  }
  return B;
}
// want_fast: 1 = partitioned whenever it applies, 0 = by size, -1 = never
// pin: factor pinned_last(A_in) instead; the launches then zero the last right-hand side entry
amg_hip_status upload_coarse(const Sparse& A_in, int want_fast, CoarseOnDev* C, bool pin) {
  Sparse A_pin;
  if (pin) A_pin = pinned_last(A_in);
  const Sparse& A = pin ? A_pin : A_in;
  C->pin = pin;
  BandFactor F;
  std::string e = band_factor(A, (size_t)8 << 30, &F);
  if (!e.empty()) return fail(AMG_HIP_EINVAL, e);
  C->n = F.n;
  C->w = F.w;
  if (F.w > 63) {
    BandWide W;
    e = band_wide_schedule(F, (size_t)16 << 30, &W);
    if (!e.empty()) return fail(AMG_HIP_EUNSUPPORTED, e);
    C->kind = COARSE_WIDE;
    HIP_TRY(upload(C->sf, W.sched_f.data(), W.sched_f.size()));
    HIP_TRY(upload(C->sb, W.sched_b.data(), W.sched_b.size()));
    HIP_TRY(upload(C->d, W.d.data(), W.d.size()));
    return AMG_HIP_OK;
  }
  if (want_fast > 0 || (want_fast == 0 && F.n >= COARSE_SPIKE_MIN_ROWS)) {
    SpikeFactor SF;
    e = spike_factor(F, &SF);
    if (e.empty()) {
      C->kind = COARSE_SPIKE;
      C->spike.reset(new SpikeOnDev);
      HIP_TRY(upload_spike(SF, C->spike.get()));
      return AMG_HIP_OK;
    }
  }
  if (band_chain_ok(F.n, F.w) && !g_no_band_chain) {
    BandChain S;
    band_chain_schedule(F, &S);
    C->kind = COARSE_CHAIN;
    HIP_TRY(upload(C->sf, S.cf.data(), S.cf.size()));
    HIP_TRY(upload(C->sb, S.cb.data(), S.cb.size()));
    HIP_TRY(upload(C->d, S.d.data(), S.d.size()));
    return AMG_HIP_OK;
  }
  BandSchedule S;
  e = band_schedule(F, &S);
  if (!e.empty()) return fail(AMG_HIP_EUNSUPPORTED, e);
  C->kind = COARSE_BAND;
  C->m = S.m;
  HIP_TRY(upload(C->sf, S.sched_f.data(), S.sched_f.size()));
  HIP_TRY(upload(C->sb, S.sched_b.data(), S.sched_b.size()));
  HIP_TRY(upload(C->d, S.d.data(), S.d.size()));
  return AMG_HIP_OK;
}
// x = A^-1 f; y: scratch of n doubles (BAND / WIDE)
// uh_out (K-BandChain only): also uh_out = uh_in + P x, the prolongation into the level above
// C.pin: f[n-1] is zeroed first (one more static node of a captured graph)
// cols > 1 (the block cycle): column c's f / y / x at c * cstride; the one-wave kinds take every column in
// one launch (one workgroup per column), K-Spike one launch per column
hipError_t launch_coarse(const CoarseOnDev& C, double* f, double* y, double* x,
                         hipStream_t st, int64_t n_h = 0, const double* uh_in = nullptr,
                         double* uh_out = nullptr, int cols = 1, int64_t cstride = 0) {
  if (C.pin) {
    const hipError_t e = launch_zero_strided(f + (C.n - 1), cstride, cols, st);
    if (e != hipSuccess) return e;
  }
  switch (C.kind) {
    case COARSE_SPIKE:
      for (int j = 0; j < cols; ++j) {
        SpikeArgs a = C.spike->a;
        a.f = f + (size_t)j * (size_t)cstride;
        a.x = x + (size_t)j * (size_t)cstride;
        const hipError_t e = launch_spike_solve(a, st);
        if (e != hipSuccess) return e;
      }
      return hipSuccess;
    case COARSE_WIDE:
      return launch_band_wide(C.n, C.w, C.sf.as<double>(), C.sb.as<double>(), C.d.as<double>(), f,
                              y, x, st, cols, cstride);
    case COARSE_CHAIN:
      return launch_band_chain(C.n, (int)C.w, C.sf.as<double>(), C.sb.as<double>(), C.d.as<double>(),
                               f, x, st, n_h, uh_in, uh_out, cols, cstride);
    default:
      return launch_band_solve(C.n, C.m, C.sf.as<double>(), C.sb.as<double>(), C.d.as<double>(),
                               f, y, x, st, cols, cstride);
  }
}

struct LexOnDev {
  LexDev d;
  DevMem row, depth, win_depth, col, val, src;
  int64_t n_sets = 0;
};

hipError_t upload_lex(const LexSchedule& S, LexOnDev* L) {
  hipError_t e;
  if ((e = upload(L->row, S.row.data(), S.row.size())) != hipSuccess) return e;
  if ((e = upload(L->depth, S.depth.data(), S.depth.size())) != hipSuccess) return e;
  if ((e = upload(L->win_depth, S.win_depth.data(), S.win_depth.size())) != hipSuccess) return e;
  if ((e = upload(L->col, S.col.data(), S.col.size())) != hipSuccess) return e;
  if ((e = upload(L->val, S.val.data(), S.val.size())) != hipSuccess) return e;
  if ((e = upload(L->src, S.src.data(), S.src.size())) != hipSuccess) return e;
  L->d.block = S.block;
  L->d.width = S.width;
  L->d.n_slots = S.n_slots;
  L->d.row = L->row.as<int32_t>();
  L->d.depth = L->depth.as<int16_t>();
  L->d.win_depth = L->win_depth.as<int32_t>();
  L->d.col = L->col.as<int32_t>();
  L->d.val = L->val.as<double>();
  L->d.src = L->src.as<int16_t>();
  L->n_sets = S.n_sets;
  return hipSuccess;
}

struct Level {
  int64_t n = 0;
  int64_t nnz_struct = 0;  // structural entries (exact zeros of the Galerkin product included)
  // host copy, what get_coefficient_matrix returns.  Device-only setup (amg_hip_create_poisson)
  // leaves it empty and keeps CSR(A) on the device instead; ensure_host_matrix() fills it on demand.
  mutable Sparse A_csc;
  DevCsr A_dev;
  hipError_t ensure_host_matrix() const {
    if (!A_csc.ptr.empty() || A_dev.n_rows <= 0) return hipSuccess;
    Sparse H;  // symmetric: the CSR arrays are the CSC arrays
    const hipError_t e = download_csr(A_dev, &H);
    if (e == hipSuccess) A_csc = std::move(H);
    return e;
  }
  DevMat A_rows;           // rows of A: residual, rss
  DevMat A_cols_own;       // CSC arrays walked as rows (column-as-row smoothers,
  bool symmetric = false;  //   smoother.hpp:101-117); aliases A_rows when bitwise equal
  const DevMat& A_cols() const { return symmetric ? A_rows : A_cols_own; }
  DevMem u, f, r, tmp;
  DevMem diag;             // a_ii (true-Jacobi smoother only)
  double cheb_lo = 0.0, cheb_hi = 0.0;  // Chebyshev smoother: interval of D^-1 A's spectrum
  DevMem cheb_d;           //   and its update vector d (r stays the residual: keep_residual)
  LineOnDev line;          // line smoother: stride, factors of T and scratch (host_only: stride only)
  AltOnDev alt;            // alternating line smoother: directions and their factors (host_only: directions only)
  // transfers to level+1 (absent on the coarsest level)
  // host copies; for the built-in LinearInterpolator they are only materialised when a
  // getter, the CSR transfer kernels or the host Galerkin product ask for them
  mutable Sparse P_csc, R_csc;
  bool lazy_linear = false;
  int64_t n_coarse = 0;
  const Sparse& P() const {
    if (lazy_linear && P_csc.ptr.empty()) P_csc = linear_P(n, n_coarse);  // interpolator.hpp:106-129
    if (tensor_stencil && P_csc.ptr.empty()) P_csc = tensor_P(tdim, dims, tmask, tsides, tper);
    if (axis >= 0 && P_csc.ptr.empty() && ensure_axis_weights() == hipSuccess)
      P_csc = axis_P_from_weights(tdim, dims, axis, axis_W.data(), axis_periodic());
    return P_csc;
  }
  const Sparse& R() const {
    if ((lazy_linear || tensor_stencil || axis >= 0) && R_csc.ptr.empty()) R_csc = transpose(P());  // :132-134
    return R_csc;
  }
  bool linear = false;
  // full coarsening (amg_hip_create_tensor): the level's grid (x fastest; on every level of such a
  // solver, the coarsest included) and whether the level's transfers are the tensor-product pair.
  // tensor_stencil: they run matrix-free (opt.stencil_transfers), and the host copies of P / R are
  // only kept while somebody needs them (the Galerkin product, a getter, the block CSR copies)
  // tmask: the axes the level's transfers coarsen (bit 0 = x, 1 = y, 2 = z): all of them, or the
  // level's mask in a semi-coarsening hierarchy (amg_hip_create_tensor_semi)
  int tdim = 0;
  int64_t dims[3] = {0, 0, 0};
  bool tensor = false, tensor_stencil = false;
  uint32_t tmask = 0;
  uint32_t tsides = 0;  // the solver's natural boundary sides (opt.natural_sides), the same on every level
  uint32_t tper = 0;    // the solver's periodic axes (amg_hip_create_tensor_periodic), the same on every level
  DevCsr P_rows, R_rows;   // CSR(P), CSR(R)
  // amg_hip_create_tensor_opdep: the one axis the level coarsens (-1: another kind of level), the
  // compact weights of its P (host_setup.hpp: axis_opdep_P) on the host and, where the transfers run
  // matrix-free (axis_stencil: K-AxisRestrict / K-AxisProlong, transfer kind 3), on the device.
  // P_csc / R_csc stay on the host; CSR(P), CSR(R) reach the device when a float or block cycle asks.
  // A level built on the device (amg_hip_create_tensor_opdep_dev: K-AxisWeights) has its weights in
  // axis_W_dev alone: ensure_axis_weights() downloads them on first use, P() / R() build the host
  // operators from them (axis_P_from_weights) when a getter or a CSR cycle asks.
  // amg_hip_create_tensor_opdep_periodic: the axis may be one of tper's, and then wraps (the seam forms)
  int axis = -1;
  bool axis_periodic() const { return axis >= 0 && ((tper >> axis) & 1u); }
  bool axis_stencil = false;
  mutable std::vector<double> axis_W;
  DevMem axis_W_dev;
  hipError_t ensure_axis_weights() const {
    if (!axis_W.empty() || !axis_W_dev.p) return hipSuccess;
    std::vector<double> w((size_t)(2 * (n - n_coarse)));
    const hipError_t e = hipMemcpy(w.data(), axis_W_dev.p, sizeof(double) * w.size(), hipMemcpyDeviceToHost);
    if (e == hipSuccess) axis_W = std::move(w);
    return e;
  }
  // exact lexicographic schedules
  std::unique_ptr<LexOnDev> lex_fwd, lex_bwd;
  int scan_C = 0, scan_ring = 0;  // > 0: the lexicographic sweeps run as K-GS-scan
  // multicolour: colour-permuted SELL-64 copy + dof of every storage row
  std::vector<int32_t> color;
  // <= 4 colours that are a function of (line parity, column class) on the level's 2-D band: the table
  // as 2-bit entries (line & 1) * 6 + class, else -1 (kernels.hip: patch_rb_kernel; classes: the
  // columns 0, 1, m-2, m-1 and the even / odd columns between them)
  int mc_ctab = -1;
  DevMem mc_aux;  // third vector of the patch colour stages when r is kept (opt.keep_residual)
  DevMem mc_color8;  // colour of every row as one byte (K-Strip, kernels.hip: mc_strip_kernel)
  int32_t n_colors = 0;
  DevMat mc_mat;
  DevMem mc_rowid;
  std::vector<int64_t> mc_start;
  DevMem mc_start_dev;  // the same offsets as int32 on the device (small levels: one-launch pass)
  bool mc_dict = false;    // ... dictionary-coded instead (K-Dict colour kernel)
  int mc_words = 0, mc_wmax = 0, mc_ntab = 0;
  DevMem mc_codes, mc_doff, mc_dval;
};

}  // namespace

// Row-block ("slab") sharding of the K-Patch levels: every rank holds the whole
// hierarchy and full-size vectors, but runs the patch kernels of levels 0..levels-1 only over
// its own grid lines plus a halo deep enough that NO exchange is needed inside those legs
// (the halo lines are recomputed redundantly: each kernel stage makes one more line at either
// end of the range stale, and the ranges below are what is left valid where it is needed).
// The level below the slab levels is all-gathered and the rest of the cycle runs replicated.
struct Slab {
  int levels = 0;               // 0: not configured
  int rank = 0, world = 1;
  int64_t lines = 0, chunk = 0, line0 = 0, line1 = 0;   // grid lines; lines per rank; owned [line0, line1)
  int halo = 0;                 // lines of level-0 u a neighbour supplies before each cycle
  std::vector<int64_t> down_lo, down_hi, up_lo, up_hi;  // lines each leg runs over, per level
  CycleGraph graph[3];          // per part (CYCLE_SLAB_DOWN .. CYCLE_SLAB_UP)
  void reset_graphs() {
    for (CycleGraph& g : graph) g.reset();
  }
};

// Block (multi-right-hand-side) cycle: per-level panels of n_l x kp doubles (row-major, entry (i, j)
// at i * kp + j; kp = k rounded up to a power of two <= 16, padded columns zero) and the plain CSR
// copies the block kernels walk.  Made at the first block call; the panels grow with kp.
struct BlockLevel {
  DevCsr rows_own, cols_own;       // CSR copies of levels whose single-vector layout is not CSR
  const DevCsr* rows = nullptr;    // rows of A (residual, Chebyshev, rss, PCG)
  const DevCsr* cols = nullptr;    // columns of A walked as rows (Jacobi); = rows when symmetric
  DevMem U, F, R, T, D;            // solution, right-hand side, residual, ping-pong, Chebyshev d
  DevMem Y;                        // K-Line's y panel (line smoothers only)
};
constexpr int BLOCK_K_MAX = 16;
struct Block {
  bool mats = false;               // the CSR copies exist
  int kp_alloc = 0;                // panel pitch the buffers were allocated for
  std::vector<BlockLevel> lv;
  DevMem cf, cy, cx;               // coarsest level as kp contiguous columns: f, scratch, x
  DevMem px, pp, pq, pb;           // PCG panels (level-0 size)
  DevMem part, dots, act;          // 1024 x 16 partials; 6 x 16 device scalars; 16 column flags
  CycleGraph graph[5];             // per log2(kp)
  void reset_graphs() {
    for (CycleGraph& g : graph) g.reset();
  }
};

// Single-precision cycle (amg_hip_apply_f32 / amg_hip_pcg_mixed): float copies of the matrix values
// the double sweep and residual of a level read (the SELL panel offsets and indices, the CSR row
// pointers and columns are the double matrix's own arrays), float level vectors, and the cycle's
// captured graph.  Made at the first call, freed with the solver, never rebuilt.
struct F32Mat {
  const DevMat* src = nullptr;  // layout and index arrays
  DevMem val;                   // src's sval (SELL), csr.val (CSR) or dval (dictionary: the pair table) as floats
};
// float copies of one K-Line factor set (LineOnDev) and its scratch vector
struct F32Line {
  DevMem dl, ip, cp, v, w, y;
  LineRefT<float> ref(const LineOnDev& D) const {
    LineRefT<float> R;
    R.n = D.n;
    R.s = D.s;
    R.dl = dl.as<float>();
    R.ip = ip.as<float>();
    R.cp = cp.as<float>();
    R.v = v.as<float>();
    R.w = w.as<float>();
    return R;
  }
};
struct F32Level {
  F32Mat rows, cols_own;
  const F32Mat* cols = nullptr;  // what the Jacobi sweep walks; = &rows on a bitwise symmetric level
  DevMem u, f, r, tmp, d;        // floats; d: Chebyshev
  DevMem pval, rval;             // CSR transfers (kind 0): values of P_rows / R_rows as floats
  // line smoothers (amg_hip_set_f32_lines): float copies of the level's double factors
  F32Line line;                  // LINE_JACOBI: Level::line
  DevMem xdl, xip, xcp;          // LINE_ALT: AltOnDev's K-LineX factors
  F32Line yz[2];                 //           AltOnDev::yz
  DevMem seam_p[3], seam_coef[3];  //         AltOnDev's K-LineSeam arrays
  LineXRefT<float> xref(const AltOnDev& D) const {
    LineXRefT<float> R;
    R.n = D.n;
    R.nx = D.len[0];
    R.dl = xdl.as<float>();
    R.ip = xip.as<float>();
    R.cp = xcp.as<float>();
    return R;
  }
  SeamRefT<float> seam(const AltOnDev& D, int d) const {
    SeamRefT<float> S;
    S.n = D.n;
    S.s = D.stride[d];
    S.m = D.len[d];
    S.p = seam_p[d].as<float>();
    S.coef = seam_coef[d].as<float>();
    return S;
  }
};
struct F32 {
  bool ready = false;
  std::vector<F32Level> lv;
  DevMem cf, cy, cx;             // coarsest system in double: f, scratch, x
  DevMem pr, pz;                 // amg_hip_pcg_mixed: r and z (doubles, level-0 size)
  CycleGraph graph;
};

// amg_hip_set_tail_fusion / AMG_HIP_TAIL_FUSION=1: K-Tail (deepest levels + coarsest solve in one
// launch).  Off by default: bit-identical, and measured 0.5 % SLOWER than one launch per step on the
// 4096^2 cycle (1282 / 1291 / 1293 against 1299 / 1301 / 1294 V-cycles/s, alternating runs).
// K-March on / off (AMG_HIP_MARCH=0: two launches of the sweep)
int g_march = [] {
  const char* e = std::getenv("AMG_HIP_MARCH");
  return (e && *e == '0') ? 0 : 1;
}();
int g_tail_fusion = [] {
  const char* e = std::getenv("AMG_HIP_TAIL_FUSION");
  return (e && *e == '1') ? 1 : 0;
}();
// amg_hip_set_periodic_device_setup / AMG_HIP_PERIODIC_DEVICE_SETUP=1: amg_hip_create_tensor_periodic_dev
// and amg_hip_create_tensor_opdep_periodic_dev build on the device.  The same solvers bit for bit; 0 by
// default only because earlier tests pin amg_hip_setup_on_device == 0 for those entry points
// ("Periodic axes", "Operator-dependent interpolation").
int g_periodic_device_setup = [] {
  const char* e = std::getenv("AMG_HIP_PERIODIC_DEVICE_SETUP");
  return (e && *e == '1') ? 1 : 0;
}();
// amg_hip_set_f32_lines / AMG_HIP_F32_LINES=1: the single-precision cycle accepts the line smoothers
// (K-LineF32).  0 by default only because earlier tests pin the refusal of the float entry points on
// line-smoother solvers ("Single-precision preconditioner").
int g_f32_lines = [] {
  const char* e = std::getenv("AMG_HIP_F32_LINES");
  return (e && *e == '1') ? 1 : 0;
}();
// amg_hip_set_f32_dict / AMG_HIP_F32_DICT=1: the single-precision cycle accepts levels stored in the
// dictionary layout (K-DictF32).  0 by default only because an earlier test pins the refusal of the float
// entry points on such a solver ("Single-precision preconditioner").
int g_f32_dict = [] {
  const char* e = std::getenv("AMG_HIP_F32_DICT");
  return (e && *e == '1') ? 1 : 0;
}();
// amg_hip_set_block_lines / AMG_HIP_BLOCK_LINES=1: the block entry points accept the line smoothers
// (K-LineBlock).  0 by default only because earlier tests pin their refusal on line-smoother solvers
// ("Block cycle").
int g_block_lines = [] {
  const char* e = std::getenv("AMG_HIP_BLOCK_LINES");
  return (e && *e == '1') ? 1 : 0;
}();
// amg_hip_set_pair_duo / AMG_HIP_PAIR_DUO=0: K-Duo (two consecutive pair levels per launch), read when
// a solver is created.  Same bits either way.
int g_pair_duo = [] {
  const char* e = std::getenv("AMG_HIP_PAIR_DUO");
  return (e && *e == '0') ? 0 : 1;
}();
int64_t g_patch_min_rows = 1000000;  // amg_hip_set_patch_min_rows (level 4 of 4096^2 has 1 048 575 rows)

// The cycle plan ("The cycle plan"): which launch form every level of the
// double-precision V-cycle takes on each leg and which of its two buffers holds its iterate when,
// chosen once per enqueue by build_cycle_plan.  The enqueue dispatches on it and the accessors read it;
// nothing else asks an eligibility predicate.  The buffers' roles are read from the plan (between_legs,
// after_up, up_target, resting): no function reached from an enqueue or a level operation assigns to, or
// swaps, a DevMem member of a Level, so a failing HIP call anywhere leaves every level as it found it.
enum LegForm : uint8_t {
  LEG_NONE,        // no launch of its own: the coarsest level (solved, not smoothed) when r is not kept
  LEG_MC_PATCH,    // multicolour smoother, colour stages as patch launches
  LEG_MC_STRIP,    // multicolour smoother, a narrow level as one strip launch
  LEG_PATCH,       // K-Patch: the whole leg in one launch
  LEG_TAIL_HEAD,   // K-Tail: this level .. L-2, the solve and the way back in one launch
  LEG_IN_TAIL,     // a level inside that launch
  LEG_DUO_FINE,    // K-Duo: the finer level of a duo (down-leg: it launches; up-leg: the coarser one does)
  LEG_DUO_COARSE,  // K-Duo: the coarser level
  LEG_PAIR,        // two sweeps of a small level in one launch
  LEG_PLAIN        // enqueue_smooth, then the residual and the restriction
};
enum ProlongBy : uint8_t {
  PROLONG_NONE,           // the coarsest level, or a level inside K-Tail
  PROLONG_LOADING,        // the level's own up-leg kernel, while it loads
  PROLONG_COARSER_SWEEP,  // the last sweep of level l+1 (plain, pair, duo or tail launch)
  PROLONG_SOLVE,          // the launch of the coarsest solve
  PROLONG_OWN_SMOOTHER,   // the first sweep of its own smoother (opt.fuse_prolong)
  PROLONG_TRANSFER        // enqueue_prolong_add
};
struct LevelPlan {
  LegForm down = LEG_NONE, up = LEG_NONE;
  int phase = 0;                       // smoother phase of a plain down-leg: 0, 1 or 3 (enqueue_smooth)
  bool xf_in = false, xf_out = false;  // K-Patch hand-over: this level / level l+1 forms its first sweep from f
  bool restrict_fused = false;         // plain down-leg: residual + restriction (+ first coarse sweep) in one launch
  ProlongBy prolong = PROLONG_NONE;    // who adds P u_{l+1} to this level
  bool up_tmp = false;                 // ... and where: tmp, else u in place
  // K-March sweeps this leg in one launch (a plain leg in phase 0 that prolongs nowhere).  Between its
  // legs the iterate of a level marched down lives in tmp for every reader and writer; the up-leg marches back
  bool march_down = false, march_up = false;
  bool home_copy() const { return march_down != march_up; }  // one leg only: the cycle ends with tmp -> u
  bool rests_tmp = false;              // the solution rests in tmp after the cycle, else in u
  bool writes_r = true;                // r is written when keep_residual is 0
};
struct CyclePlan {
  std::vector<LevelPlan> lv;
  int tail_first = -1;      // the K-Tail head, or -1
  bool seam = false;        // amg_hip_vcycles(n >= 2) runs the seam sequence
  bool zero_known = false;  // coarse pre-smoothing starts from u == 0 without reading it
};

struct amg_hip_solver {
  amg_hip_options opt;
  int64_t patch_min_rows = g_patch_min_rows;  // the process-wide value when the solver was made
  int patch_xf = g_patch_xf;                  // likewise
  int patch_tall = g_patch_tall;              // likewise
  int patch_seam = g_patch_seam;              // likewise
  int pair_duo = g_pair_duo;                  // likewise
  // the plan of the whole cycle (or slab tail) enqueued last (a captured graph keeps what it was
  // captured with): where a level rests follows what ran, not switches flipped since
  CyclePlan plan;
  bool plan_kept = false;
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = true;
  std::vector<Level> lv;
  bool device_setup = false;  // the hierarchy was built by build_poisson_device (amg_hip_setup_on_device)
  CoarseOnDev coarse;  // coarsest level factor
  DevMem scratch;   // 1024 doubles + 1 result
  DevMem pcg_x, pcg_p, pcg_q, pcg_b;  // PCG work vectors (allocated on first use)
  bool project_mean = false;  // amg_hip_set_mean_projection: the PCG drivers project onto the complement of the constants
  CycleGraph graph;  // the whole cycle
  double cycle_bytes = 0, fine_sweep_bytes = 0;
  // bytes the launches of one V-cycle HAVE TO move (what each kernel reads and writes once in the
  // layout it really streams), summed while the cycle is enqueued (CycleCtx); [part] as enqueue_vcycle's
  // [4]: one steady-state seam cycle (seam launch + levels 1 .. L-1; amg_hip_vcycles), [5]: its head and finish
  double must_move[6] = {0, 0, 0, 0, 0, 0};
  // K-Patch seam (amg_hip_vcycles with n >= 2, patch_seam_ok): the captured pieces -- head and seam
  // cycle per level-0 buffer handed over in (0: tmp, 1: r), the finish
  CycleGraph seam_graph[5];
  Slab slab;
  Block blk;
  F32 f32;

  // every captured graph goes before the stream it was captured on (members die after this body)
  ~amg_hip_solver() {
    f32.graph.reset();
    blk.reset_graphs();
    slab.reset_graphs();
    for (CycleGraph& g : seam_graph) g.reset();
    graph.reset();
    if (stream && own_stream) (void)hipStreamDestroy(stream);
  }
};

namespace {

void layout_of(const DevMat& A, int32_t* layout, int64_t* matrix_stream_bytes);  // below
// matrix stream of one pass over a level matrix in its device layout (dictionary: 1 B row type per
// row + tables; SELL / CSR: indices + values), the figure amg_hip_level_layout reports
double mat_bytes(const DevMat& A) {
  int64_t b = 0;
  layout_of(A, nullptr, &b);
  return (double)b;
}

// What a step of a cycle enqueues on, and the bytes its launches have to move.  launch = false is the
// dry run of amg_hip_block_must_move / amg_hip_f32_must_move: count, launch nothing (the double cycle has none).
struct StepCtx {
  hipStream_t st = nullptr;
  bool launch = true;
  double once = 0;     // bytes moved once per launch (the double and the float cycle count all of their bytes here)
  double per_col = 0;  // bytes per column of a block panel: k columns have to move once + k * per_col
  void count(double o, double c = 0.0) {
    once += o;
    per_col += c;
  }
};
// A level's iterate and its second buffer as one step sees them: u and tmp of the Level, or the two
// the other way round where the plan says the iterate lives in tmp.
struct LevelVecs { double *u, *tmp; };
LevelVecs level_vecs(const Level& L, bool in_tmp) {
  double *u = L.u.as<double>(), *t = L.tmp.as<double>();
  return in_tmp ? LevelVecs{t, u} : LevelVecs{u, t};
}

// ---- smoother on one level --------------------------------------------------
amg_hip_status enqueue_multicolor(StepCtx& X, amg_hip_solver* s, Level& L, double* u, bool again);

// full coarsening: level l (grid d) has an axis that cannot be coarsened, so level l + 1 is not possible
std::string tensor_level_error(int l, const int64_t d[3]) {
  return "level " + std::to_string(l + 1) + " is not possible: level " + std::to_string(l) + " is a " +
         std::to_string(d[0]) + " x " + std::to_string(d[1]) + " x " + std::to_string(d[2]) +
         " grid and an axis of fewer than 2 points cannot be coarsened; reduce `n_levels`";
}

// phase 0: u_l is arbitrary.  phase 1: u_l is known to be zero (pre-smoothing of a
// coarse level, multigrid.hpp:278).  phase 2: u_l still lacks the correction
// P u_{l+1} (multigrid.hpp:294-296), the smoother must apply it.  Only the true
// Jacobi smoother has shortcuts for phases 1/2; callers fall back otherwise.
bool jacobi_fuses_zero(const amg_hip_solver* s) {
  return s->opt.smoother == AMG_HIP_SM_JACOBI && !s->opt.no_fusion && s->opt.smoother_iters >= 1;
}
bool jacobi_fuses_prolong(const amg_hip_solver* s, int l) {
  const Level& L = s->lv[l];
  // measured slower than the separate prolongation kernel (3 gathers per entry:
  // 337 vs 248+70 us on the 4096^2 fine level), so only on request
  return s->opt.fuse_prolong && jacobi_fuses_zero(s) && L.linear && s->opt.stencil_transfers &&
         L.A_cols().sell;
}

// Fusions of the true-Jacobi V-cycle across a level boundary (kernels.hip, "fused
// forms"): both need the dictionary-coded layout and the matrix-free linear transfers.
// down: residual of level l + restriction + first (from-zero) sweep of level l+1
bool fuses_resid_restrict(const amg_hip_solver* s, int l) {
  if (l + 1 >= (int)s->lv.size()) return false;
  const Level& L = s->lv[l];
  if (s->opt.no_fusion || !L.linear || !s->opt.stencil_transfers || !L.A_rows.dict ||
      L.A_rows.dict_shift != 0)
    return false;
  // true Jacobi: the kernel also does the first coarse sweep and needs the coarse diagonal
  return !jacobi_fuses_zero(s) || s->lv[l + 1].diag.p != nullptr;
}
// K-Patch: the whole down-leg / up-leg of a big level in one launch each (kernels.hip).
// Levels 0 .. k of a 2+2 true-Jacobi cycle whose matrices are row-typed dictionaries with a
// 2-D band (the finer level's kernel hands the first sweep of the next one over).
bool patch_level_ok(const amg_hip_solver* s, int l) {
  // needs a smoothed coarser level (a window's last level is one: it is smoothed by the tail solver)
  if (l < 0 || l + (s->opt.window ? 1 : 2) >= (int)s->lv.size()) return false;
  if (!(jacobi_fuses_zero(s) && !s->opt.fuse_prolong && s->opt.smoother_iters == 2 && s->opt.stencil_transfers))
    return false;
  for (int q = 0; q <= l; ++q) {  // this level and every finer one
    const Level& L = s->lv[q];
    const DevMat& A = L.A_rows;
    if (!(L.symmetric && A.dict && A.dict_shift == 0 && A.patch && L.linear && L.n >= s->patch_min_rows &&
          s->lv[q + 1].diag.p != nullptr))
      return false;
  }
  return true;
}
// Halo rings of a K-Patch Jacobi leg of this solver (first_down: the level-0 down-leg): the geometry of
// the launch AND of the flag arrays handed to it (DevMat::patch_ref).  Tall legs off: the three-ring
// frame of 42 lines everywhere.
int patch_rings(const amg_hip_solver* s, bool first_down) {
  return s->patch_tall ? patch_leg_rings(first_down) : 3;
}
// The hand-over between two K-Patch levels: the down-leg of level l + 1 forms its first sweep from
// f_{l+1} (the xf form of patch_down_kernel), so the down-leg of level l stores f_{l+1} alone.  ONE
// predicate decides both sides of the pair, for whole-level and ranged (slab, window) launches alike.
bool patch_xf_pair(const amg_hip_solver* s, int l) {
  return s->patch_xf && patch_level_ok(s, l) && patch_level_ok(s, l + 1);
}

// The seam between two cycles run back to back (amg_hip_vcycles with n >= 2): the level-0 up-leg of one
// and the level-0 down-leg of the next as ONE launch (kernels.hip: patch_seam_kernel), so the vector
// between them is neither stored nor loaded.  ONE predicate: levels 0 and 1 are K-Patch Jacobi levels
// with the hand-over between them (which implies the true-Jacobi 2+2 smoother with fusion on, and at
// least three levels), the cycle is whole, the residual is not kept (the level's r is then free: the
// handed-over vector alternates between tmp and r), and level 0 is of the kernel's 5-point kind.
enum { SEAM_OFF = 0, SEAM_HEAD = 1, SEAM_CYCLE = 2, SEAM_FINISH = 3 };
bool patch_seam_ok(const amg_hip_solver* s) {
  if (!s->patch_seam || s->lv.size() < 2 || s->opt.window || s->slab.levels != 0 || s->opt.keep_residual ||
      s->opt.no_fusion || s->opt.smoother != AMG_HIP_SM_JACOBI)
    return false;
  const Level& L = s->lv[0];
  return patch_xf_pair(s, 0) && patch_un(L.A_rows.patch_un) == 5 && L.A_rows.patch_flags5.p != nullptr &&
         L.r.p != nullptr && L.r.bytes >= sizeof(double) * (size_t)L.n;
}
// the level-0 vector a piece of the seam sequence hands over: tmp or r
double* seam_buf(amg_hip_solver* s, int which) {
  return which ? s->lv[0].r.as<double>() : s->lv[0].tmp.as<double>();
}

// Multicolour smoother on a level whose colours repeat on the 2 x 2 cells of its 2-D band (the
// checkerboard of the 5-point level, line parity, the product colouring of the 9-point levels): the
// symmetric passes as patch stages, the residual + restriction and the prolongation fused into them
// (kernels.hip: patch_rb_kernel)
bool mc_patch_ok(const amg_hip_solver* s, int l) {
  if (l < 0 || l + 1 >= (int)s->lv.size()) return false;
  const Level& L = s->lv[l];
  const DevMat& A = L.A_rows;
  return s->opt.smoother == AMG_HIP_SM_MULTICOLOR_GS && s->opt.smoother_iters >= 1 && !s->opt.no_fusion &&
         L.symmetric && A.dict && A.dict_shift == 0 && A.patch && L.linear && s->opt.stencil_transfers &&
         L.n >= s->patch_min_rows && L.mc_ctab >= 0 && s->lv[l + 1].n >= 2 &&
         (!s->opt.keep_residual || L.mc_aux.p != nullptr);
}
// The colour stages of smoother_iters symmetric passes (0 .. nc-1, nc-1 .. 0 each).  A colour that
// directly follows itself is dropped: its rows read no row of their own colour (that is what the
// colouring means; explicit zeros add +-0.0), so the repeat would store the bits already there.
static std::vector<int> mc_sequence(int nc, int iters) {
  std::vector<int> q;
  for (int it = 0; it < iters; ++it) {
    for (int c = 0; c < nc; ++c)
      if (q.empty() || q.back() != c) q.push_back(c);
    for (int c = nc - 1; c >= 0; --c)
      if (q.back() != c) q.push_back(c);
  }
  return q;
}
// The launches of one level and cycle in the patch form: the down-leg (the last launch carries the
// residual + restriction and at most patch_rb_max_stages(true) stages), then the up-leg (the first
// launch prolongs while loading).  A launch cannot write the vector it reads (tiles overlap), so
// the level vector travels u -> tmp -> r -> tmp ... -> u (r, or mc_aux when r is kept).
struct McLaunch {
  uint32_t stages = 0;
  bool prolong = false, tail = false;
  double *in = nullptr, *out = nullptr;
};
static std::vector<McLaunch> mc_plan(amg_hip_solver* s, int l, int* n_down) {
  Level& L = s->lv[l];
  const std::vector<int> q = mc_sequence(L.n_colors, s->opt.smoother_iters);
  const int n = (int)q.size();
  std::vector<McLaunch> P;
  auto chunks = [&](int from, int count, int cap, bool prolong_first) {
    if (count <= 0) return;
    const int k = (count + cap - 1) / cap;
    int at = from;
    for (int c = 0; c < k; ++c) {
      const int len = count / k + (c < count % k ? 1 : 0);
      McLaunch M;
      M.stages = patch_rb_stages(q.data() + at, len);
      M.prolong = prolong_first && c == 0;
      P.push_back(M);
      at += len;
    }
  };
  const int tail_cnt = std::min(n, patch_rb_max_stages(true));
  chunks(0, n - tail_cnt, patch_rb_max_stages(false), false);
  {
    McLaunch M;
    M.stages = patch_rb_stages(q.data() + (n - tail_cnt), tail_cnt);
    M.tail = true;
    P.push_back(M);
  }
  *n_down = (int)P.size();
  chunks(0, n, patch_rb_max_stages(false), true);
  double* third = s->opt.keep_residual ? L.mc_aux.as<double>() : L.r.as<double>();
  double* cur = L.u.as<double>();
  for (size_t i = 0; i < P.size(); ++i) {
    P[i].in = cur;
    P[i].out = i + 1 == P.size() ? L.u.as<double>() : ((i & 1) ? third : L.tmp.as<double>());
    cur = P[i].out;
  }
  return P;
}

// up: last post-smoothing sweep of level l+1 + prolongation into level l
bool fuses_jacobi_prolong(const amg_hip_solver* s, int l) {
  if (l + 2 >= (int)s->lv.size()) return false;  // the coarsest level is solved, not smoothed
  if (patch_level_ok(s, l)) return false;  // a patch level prolongs into itself while loading
  const Level& L = s->lv[l];
  const DevMat& AC = s->lv[l + 1].A_cols();
  return jacobi_fuses_zero(s) && !jacobi_fuses_prolong(s, l) && L.linear &&
         s->opt.stencil_transfers && AC.dict && AC.dict_shift == 0;
}

// two sweeps in one launch (kernels.hip: dict_pair_*_kernel): small, narrow-band,
// symmetric levels of the 2+2 true-Jacobi cycle
bool pair_level_ok(const amg_hip_solver* s, int l) {
  if (l < 1 || l + 1 >= (int)s->lv.size()) return false;
  const Level& L = s->lv[l];
  const DevMat& A = L.A_rows;
  return jacobi_fuses_zero(s) && s->opt.smoother_iters == 2 && L.symmetric && A.dict &&
         A.dict_shift == 0 && fuses_resid_restrict(s, l) &&
         dict_pair_ok(L.n, A.dict_ref(), A.dict_hb, L.u.p, L.f.p, L.tmp.p);
}
bool pair_up_ok(const amg_hip_solver* s, int l) {  // its second sweep prolongs into level l-1
  return pair_level_ok(s, l) && fuses_jacobi_prolong(s, l - 1);
}

// K-Tail: first level lt such that the levels lt .. L-2, the coarsest solve and the prolongation
// into lt - 1 run as ONE launch (kernels.hip: tail_kernel), or -1.
int tail_from(const amg_hip_solver* s) {
  const int nl = (int)s->lv.size();
  if (!g_tail_fusion || s->opt.keep_residual || s->opt.window || nl < 3 || s->coarse.kind != COARSE_CHAIN || s->coarse.pin ||
      s->coarse.n > tail_max_coarse())
    return -1;
  int lt = nl - 1;
  while (lt - 1 >= 1 && nl - 1 - (lt - 1) <= TAIL_LEVELS_MAX) {
    const int l = lt - 1;
    const Level& L = s->lv[l];
    if (!(pair_level_ok(s, l) && pair_up_ok(s, l) && tail_level_ok(L.n, L.A_rows.dict_ref(), L.A_rows.dict_hb) &&
          L.diag.p && s->lv[l + 1].diag.p))
      break;
    lt = l;
  }
  // the level vectors live in LDS: drop levels from the top until the launch fits
  for (; lt <= nl - 2; ++lt) {
    TailRef T;
    std::memset(&T, 0, sizeof(T));
    T.nlev = nl - 1 - lt;
    for (int q = 0; q < T.nlev; ++q) T.L[q].n = (int)s->lv[lt + q].n;
    T.nc = (int)s->coarse.n;
    T.wc = (int)s->coarse.w;
    if (tail_lds_bytes(T) <= tail_lds_capacity()) return lt;
  }
  return -1;
}

// K-Duo: the pair launches of levels l and l+1 as ONE launch per leg (kernels.hip: dict_duo_*_kernel).
// Both are pair levels on both legs, neither is a K-Patch level or belongs to K-Tail, both lie on one side of a slab cut,
// the kernels exist for their row lengths and the windows fit.
static bool duo_can(const amg_hip_solver* s, int l, int tail_lt) {
  const int nl = (int)s->lv.size();
  if (!s->pair_duo || s->opt.no_fusion || s->opt.window || l < 1 || l + 2 >= nl) return false;
  if (s->slab.levels > 0 && l < s->slab.levels) return false;  // the parts below the cut run level by level
  if (tail_lt >= 0 && l + 1 >= tail_lt) return false;
  if (patch_level_ok(s, l)) return false;  // K-Patch comes first (a K-Patch level l+1 makes l one too)
  if (!(pair_level_ok(s, l) && pair_level_ok(s, l + 1) && pair_up_ok(s, l) && pair_up_ok(s, l + 1))) return false;
  const Level& L0 = s->lv[l];
  const Level& L1 = s->lv[l + 1];
  const Level& L2 = s->lv[l + 2];
  return L1.diag.p && L2.diag.p &&
         dict_duo_ok(L0.n, L0.A_rows.dict_ref(), L0.A_rows.dict_hb, L1.n, L1.A_rows.dict_ref(), L1.A_rows.dict_hb, L2.n);
}
// partner[l] = the other level of l's duo, or -1: greedy from the finest pair level, a leftover
// single level keeps the pair form
static std::vector<int> duo_pairing(const amg_hip_solver* s, int tail_lt) {
  const int nl = (int)s->lv.size();
  std::vector<int> partner((size_t)nl, -1);
  if (!s->pair_duo) return partner;
  for (int l = 1; l + 2 < nl;) {
    if (duo_can(s, l, tail_lt)) {
      partner[(size_t)l] = l + 1;
      partner[(size_t)l + 1] = l;
      l += 2;
    } else {
      ++l;
    }
  }
  return partner;
}

// K-March: the two plain Jacobi sweeps of a 3-D 7-point level as ONE launch from the level's iterate
// v.u into its other buffer v.tmp (kernels.hip: march_kernel); the plan says which leg runs it and
// where the iterate lives afterwards (LevelPlan::march_down).  Fills the launch's arguments; the plan
// builder also takes the answer as the level's eligibility (finish_dict): the 7-point offsets of one
// interior type, n a multiple of the plane, and no row on a line / plane edge coupling across it.
static bool march_fill(const amg_hip_solver* s, int l, LevelVecs v, MarchRef* R) {
  const Level& L = s->lv[l];
  const DevMat& A = L.A_cols();
  if (!(s->opt.smoother == AMG_HIP_SM_JACOBI && s->opt.smoother_iters == 2 && !s->opt.no_fusion && !s->opt.window &&
        s->slab.levels == 0 && A.dict && A.dict_typed && A.march_ntypes > 0 && A.dmarch.p && A.march_m > 0 &&
        L.n % A.march_M == 0 && A.march_M % A.march_m == 0 && g_march))
    return false;
  R->m = A.march_m;
  R->lines = A.march_M / A.march_m;
  R->planes = (int)(L.n / A.march_M);
  R->ntypes = A.march_ntypes;
  R->tint = A.march_tint;
  R->omega = s->opt.omega;
  R->dint = A.march_dint;
  for (int u = 0; u < 6; ++u) R->wint[u] = A.march_wint[u];
  R->wtab = A.dmarch.as<double>();
  R->rtype = A.drtype.as<uint8_t>();
  R->f = L.f.as<double>();
  R->x = v.u;
  R->out = v.tmp;
  R->chunk_planes = 1;
  return march_ok(*R);
}
// phase 3: the first sweep was already done by the fused kernel of the finer level
// (result in tmp).
struct Sweep {
  int phase = 0;
  bool march = false;    // the plan sweeps this leg with K-March: v.u -> v.tmp (LevelPlan::march_down / march_up)
  bool reverse = false;  // the application of the up-leg (AMG_HIP_SM_LINE_ALT runs its directions in descending order)
  const double* coarse_u = nullptr;  // phase 2: u_{l+1}
  const double* fine_u = nullptr;    // set: the last sweep also adds P u_l to level l-1, fine_out = fine_u + P u_l
  double* fine_out = nullptr;
};
// One smoothing application on level l, on the iterate v.u with v.tmp as the second buffer.
amg_hip_status enqueue_smooth(StepCtx& X, amg_hip_solver* s, int l, LevelVecs v, const Sweep& w = Sweep()) {
  Level& L = s->lv[l];
  hipStream_t st = X.st;
  const int iters = s->opt.smoother_iters, phase = w.phase;
  switch (s->opt.smoother) {
    case AMG_HIP_SM_SPGS:
      // forward + backward sweep: matrix, f, u in, u out each (the scan form's pre-pass also
      // writes and re-reads one number per row: + 16 n)
      X.count(iters * 2.0 * (mat_bytes(L.A_rows) + 24.0 * L.n + (L.scan_C > 0 ? 16.0 * L.n : 0.0)));
      for (int it = 0; it < iters; ++it) {
        if (L.scan_C > 0) {  // line-scan form (kernels.hip: K-GS-scan)
          const DictRef D = L.A_rows.dict_ref();
          HIP_TRY(launch_gs_scan(L.n, D, L.f.as<double>(), v.u, v.tmp, false, 0,
                                 1.0, L.scan_C, L.scan_ring, st));
          HIP_TRY(launch_gs_scan(L.n, D, L.f.as<double>(), v.u, v.tmp, true, 0,
                                 1.0, L.scan_C, L.scan_ring, st));
          continue;
        }
        HIP_TRY(launch_gs_lex(L.lex_fwd->d, L.f.as<double>(), v.u, 0, 1.0, st));
        HIP_TRY(launch_gs_lex(L.lex_bwd->d, L.f.as<double>(), v.u, 0, 1.0, st));
      }
      return AMG_HIP_OK;
    case AMG_HIP_SM_REF_JACOBI:
    case AMG_HIP_SM_SOR: {
      const int mode = s->opt.smoother == AMG_HIP_SM_SOR ? 2 : 1;
      X.count(iters * (mat_bytes(L.A_rows) + 24.0 * L.n + (L.scan_C > 0 ? 16.0 * L.n : 0.0)));
      for (int it = 0; it < iters; ++it) {
        if (L.scan_C > 0) {
          HIP_TRY(launch_gs_scan(L.n, L.A_rows.dict_ref(), L.f.as<double>(), v.u,
                                 v.tmp, false, mode, s->opt.omega, L.scan_C, L.scan_ring, st));
          continue;
        }
        HIP_TRY(launch_gs_lex(L.lex_fwd->d, L.f.as<double>(), v.u, mode,
                              s->opt.omega, st));
      }
      return AMG_HIP_OK;
    }
    case AMG_HIP_SM_JACOBI: {
      const DevMat& A = L.A_cols();
      double* a = v.u;
      double* b = v.tmp;
      int it = 0;
      if (w.march) {  // both sweeps in one pass
        MarchRef R;
        (void)march_fill(s, l, v, &R);
        HIP_TRY(launch_march(R, st));
        X.count(mat_bytes(A) + 24.0 * L.n);
        return AMG_HIP_OK;
      }
      if (phase == 3) {
        std::swap(a, b);
        it = 1;
      } else if (phase == 1 && jacobi_fuses_zero(s)) {
        HIP_TRY(launch_jacobi_from_zero(L.n, L.diag.as<double>(), L.f.as<double>(), b,
                                        s->opt.omega, st));
        X.count(24.0 * L.n);  // diagonal, f, out
        std::swap(a, b);
        it = 1;
      } else if (phase == 2) {  // (asked for only where the plan has PROLONG_OWN_SMOOTHER)
        const Level& C = s->lv[l + 1];
        HIP_TRY(launch_sell_jacobi_prolong(A.n_rows, A.idx16, A.soff.as<int64_t>(),
                                           A.scol.p, A.sval.as<double>(), a,
                                           w.coarse_u, C.n, L.f.as<double>(), b,
                                           s->opt.omega, st));
        X.count(mat_bytes(A) + 24.0 * L.n + 8.0 * C.n);
        std::swap(a, b);
        it = 1;
      }
      for (; it < iters; ++it) {
        if (w.fine_u && it == iters - 1) {
          const Level& F = s->lv[l - 1];
          HIP_TRY(launch_dict_jacobi_prolong(A.n_rows, A.dict_ref(), a, L.f.as<double>(), b,
                                             s->opt.omega, F.n, w.fine_u, w.fine_out, st));
          X.count(mat_bytes(A) + 24.0 * L.n + 16.0 * F.n);  // sweep + u_F in, u_F + P u out
        } else {
          HIP_TRY(launch_mat(CSR_JACOBI, A, a, L.f.as<double>(), b, s->opt.omega, st));
          X.count(mat_bytes(A) + 24.0 * L.n);  // matrix, f, x, out
        }
        std::swap(a, b);
      }
      if (iters & 1) {  // result sits in tmp: bring it home (keeps the graph static)
        HIP_TRY(hipMemcpyAsync(v.u, v.tmp, sizeof(double) * L.n,
                               hipMemcpyDeviceToDevice, st));
        X.count(16.0 * L.n);
      }
      return AMG_HIP_OK;
    }
    case AMG_HIP_SM_MULTICOLOR_GS:
      for (int it = 0; it < iters; ++it) {
        amg_hip_status r = enqueue_multicolor(X, s, L, v.u, it > 0);
        if (r != AMG_HIP_OK) return r;
      }
      return AMG_HIP_OK;
    case AMG_HIP_SM_CHEBYSHEV: {
      // iters applications of the degree-k polynomial, each k steps from step 0 (phases 1 / 2 have
      // no shortcut here: u is read as it is).  The level vector ping-pongs u -> tmp -> u ...
      const DevMat& A = L.A_rows;
      return cheb_steps(
          L.cheb_lo, L.cheb_hi, iters, s->opt.cheb_degree, v.u, v.tmp,
          [&](double alpha, double beta, bool first, bool last, double* a, double* b) {
            const ChebStep c{L.cheb_d.as<double>(), alpha, beta, first, last};
            HIP_TRY(launch_mat_cheb(A, a, L.f.as<double>(), b, c, st));
            // matrix, f, x, out; d written (not on the last step) and read (not on the first)
            X.count(mat_bytes(A) + 24.0 * L.n + (first ? 0.0 : 8.0 * L.n) + (last ? 0.0 : 8.0 * L.n));
            return AMG_HIP_OK;
          },
          [&] {
            HIP_TRY(hipMemcpyAsync(v.u, v.tmp, sizeof(double) * L.n, hipMemcpyDeviceToDevice, st));
            X.count(16.0 * L.n);
            return AMG_HIP_OK;
          });
    }
    case AMG_HIP_SM_LINE_JACOBI:
    case AMG_HIP_SM_LINE_ALT: {
      // a sub-sweep: the residual of the current u into tmp, then the line solve adds omega T^-1 tmp
      // to u in place (phases 1 / 2 have no shortcut: u is read as it is); plain launches, r stays the
      // cycle's residual.  LINE_ALT: one sub-sweep per direction
      const DevMat& A = L.A_rows;
      const bool alt = s->opt.smoother == AMG_HIP_SM_LINE_ALT;
      return line_subsweeps(iters, line_dirs(s->opt.smoother, L.alt), w.reverse, [&](int d) {
        HIP_TRY(alt ? launch_alt_subsweep(A, L.alt, d, v.u, L.f.as<double>(), v.tmp,
                                          s->opt.omega, st)
                    : launch_line_sweep(A, L.line, v.u, L.f.as<double>(), v.tmp,
                                        s->opt.omega, st));
        // matrix, f, u, r; the line solve
        X.count(mat_bytes(A) + 24.0 * L.n + (alt ? L.alt.solve_bytes(d) : L.line.solve_bytes()));
        return AMG_HIP_OK;
      });
    }
  }
  return fail(AMG_HIP_EINVAL, "unknown smoother kind");
}

// K-Strip: the whole leg of a narrow multicolour level (below the K-Patch pitch) in one launch
// over strips of rows.  *T_out: rows per strip -- about n / 256 (one wave of workgroups), within
// what the LDS window leaves after the halo of (stages + 1) half-bandwidths on either side.
static bool mc_strip_rows(const amg_hip_solver* s, int l, int* T_out, int* nst_out);
bool mc_strip_ok(const amg_hip_solver* s, int l) {
  if (l < 0 || l + 1 >= (int)s->lv.size()) return false;
  const Level& L = s->lv[l];
  const DevMat& A = L.A_rows;
  int T = 0, nst = 0;
  return s->opt.smoother == AMG_HIP_SM_MULTICOLOR_GS && s->opt.smoother_iters >= 1 && !s->opt.no_fusion &&
         L.symmetric && A.dict && A.dict_typed && A.dict_shift == 0 && L.linear && s->opt.stencil_transfers &&
         L.mc_color8.p != nullptr && L.n_colors >= 1 && L.n_colors <= 15 && s->lv[l + 1].n >= 1 && L.n >= 2 &&
         !mc_patch_ok(s, l) && mc_strip_rows(s, l, &T, &nst);
}
// the strip geometry of a level: rows per strip and colour stages; false where no strip fits
static bool mc_strip_rows(const amg_hip_solver* s, int l, int* T_out, int* nst_out) {
  const Level& L = s->lv[l];
  const DevMat& A = L.A_rows;
  const int nst = 2 * L.n_colors * s->opt.smoother_iters - (2 * s->opt.smoother_iters - 1);  // mc_sequence
  if (nst < 1 || nst > 16) return false;
  const int hbw = (A.dict_hb + 1) & ~1;
  const int64_t T_max = ((int64_t)strip_window_max() - 2 - 2 * (int64_t)(nst + 1) * std::max(hbw, 2)) & ~(int64_t)1;
  if (T_max < 256) return false;
  int64_t T = ((L.n + 255) / 256 + 1) & ~(int64_t)1;
  T = std::min<int64_t>(std::max<int64_t>(T, 256), T_max);
  *T_out = (int)T;
  *nst_out = nst;
  return true;
}
static StripRef mc_strip_ref(amg_hip_solver* s, int l) {
  Level& L = s->lv[l];
  StripRef R;
  int T = 0, nst = 0;
  (void)mc_strip_rows(s, l, &T, &nst);
  const std::vector<int> q = mc_sequence(L.n_colors, s->opt.smoother_iters);
  R.n = (int)L.n;
  R.nH = (int)s->lv[l + 1].n;
  R.T = T;
  R.hbw = std::max((L.A_rows.dict_hb + 1) & ~1, 2);
  R.nst = (int)q.size();
  for (size_t i = 0; i < q.size() && i < 16; ++i) R.stages |= (uint64_t)(q[i] & 15) << (4 * i);
  R.color = L.mc_color8.as<uint8_t>();
  R.f = L.f.as<double>();
  return R;
}

// ---- the cycle plan -----------------------------------------------------------
// part: the whole cycle, or one of the three pieces a slab-sharded cycle is cut into at its two
// exchange points (struct Slab): the down-legs of the slab levels over this rank's lines, the
// replicated rest below them (it begins by redoing the from-zero sweep of its first level on the
// gathered right-hand side, unless that level is a K-Patch level that forms the sweep itself: the
// hand-over), the up-legs of the slab levels.
enum { CYCLE_ALL = 0, CYCLE_SLAB_DOWN = 1, CYCLE_SLAB_TAIL = 2, CYCLE_SLAB_UP = 3 };

// The ONE place that chooses launch forms: a pure host function of the hierarchy and the options as set-up
// left them (the process-wide switches as they stand now included), the part and the seam piece; it reads
// nothing that an enqueue writes.  It walks the levels once down and once up, in priority order (first
// match): multicolour patch, multicolour strip, K-Patch, K-Tail, K-Duo, pair, plain.  Every level gets an
// entry whatever the part; the enqueue walks the part's range.
CyclePlan build_cycle_plan(const amg_hip_solver* s, int part, int piece) {
  const int nl = (int)s->lv.size();
  CyclePlan P;
  P.lv.resize((size_t)nl);
  if (s->opt.host_only) return P;  // no device cycle: nothing fused, everything rests in u
  const bool whole = part == CYCLE_ALL || part == CYCLE_SLAB_TAIL;
  const int k = s->slab.levels;
  const bool keep = s->opt.keep_residual != 0;
  P.zero_known = jacobi_fuses_zero(s);
  P.seam = patch_seam_ok(s);
  // K-Tail and K-Duo only where both levels lie inside the part
  const int tail_lt = whole ? tail_from(s) : -1;
  const std::vector<int> duo = whole ? duo_pairing(s, tail_lt) : std::vector<int>((size_t)nl, -1);
  // K-March only in the stand-alone whole cycle, which sweeps a level on both legs
  const bool march_cycle = part == CYCLE_ALL && piece == SEAM_OFF;
  for (int l = 0; l < nl; ++l) {
    LevelPlan& Q = P.lv[(size_t)l];
    Q.up_tmp = pair_up_ok(s, l);
    Q.writes_r = !(fuses_resid_restrict(s, l) || patch_level_ok(s, l) || mc_patch_ok(s, l) || mc_strip_ok(s, l) ||
                   (l == nl - 1 && l > 0));
  }
  // down: first_sweep_done = the launch of the finer level also did this level's first sweep (into tmp)
  bool first_sweep_done = false;
  for (int l = 0; l < nl; ++l) {
    LevelPlan& Q = P.lv[(size_t)l];
    if (part == CYCLE_SLAB_TAIL && l == k) first_sweep_done = true;  // redone on the gathered right-hand side
    // On the coarsest level the reference smooths and forms the residual, then overwrites
    // u with the direct solve of the level's rhs (multigrid.hpp:268-274, :287-288): unless
    // the residual is to be kept, neither has an observable effect.
    if (l == nl - 1 && nl > 1 && !keep) break;
    if (mc_patch_ok(s, l) || mc_strip_ok(s, l)) {
      Q.down = mc_patch_ok(s, l) ? LEG_MC_PATCH : LEG_MC_STRIP;
      first_sweep_done = false;
    } else if (patch_level_ok(s, l)) {
      Q.down = LEG_PATCH;
      Q.xf_in = l >= 1 && patch_xf_pair(s, l - 1);
      Q.xf_out = patch_xf_pair(s, l);
      first_sweep_done = true;
    } else if (first_sweep_done && l == tail_lt) {
      for (int q = l; q < nl; ++q) P.lv[(size_t)q].down = P.lv[(size_t)q].up = LEG_IN_TAIL;
      Q.down = LEG_TAIL_HEAD;
      P.tail_first = l;
      break;
    } else if (first_sweep_done && duo[(size_t)l] == l + 1) {
      Q.down = LEG_DUO_FINE;
      P.lv[(size_t)++l].down = LEG_DUO_COARSE;  // first_sweep_done stays true for level l+2
    } else if (first_sweep_done && pair_level_ok(s, l)) {
      Q.down = LEG_PAIR;  // first_sweep_done stays true for level l+1
    } else {
      Q.down = LEG_PLAIN;
      Q.phase = first_sweep_done ? 3 : (l >= 1 && P.zero_known) ? 1 : 0;
      Q.restrict_fused = fuses_resid_restrict(s, l);
      first_sweep_done = Q.restrict_fused && P.zero_known;
    }
  }
  // up.  The coarsest solve prolongs into level L-2 (one launch less) where no other launch does
  const int lp = nl - 2;
  const bool solve_prolongs =
      P.tail_first < 0 && lp >= 0 && s->coarse.kind == COARSE_CHAIN && !s->opt.no_fusion && s->lv[lp].linear &&
      s->opt.stencil_transfers && !mc_patch_ok(s, lp) && !mc_strip_ok(s, lp) && !patch_level_ok(s, lp) &&
      !jacobi_fuses_prolong(s, lp) && !fuses_jacobi_prolong(s, lp) &&
      (part == CYCLE_ALL || (part == CYCLE_SLAB_TAIL && lp >= k));
  for (int l = P.tail_first >= 0 ? P.tail_first - 1 : nl - 2; l >= 0; --l) {
    LevelPlan& Q = P.lv[(size_t)l];
    if (mc_patch_ok(s, l) || mc_strip_ok(s, l)) {
      Q.up = mc_patch_ok(s, l) ? LEG_MC_PATCH : LEG_MC_STRIP;
      Q.prolong = PROLONG_LOADING;
    } else if (patch_level_ok(s, l)) {
      // level 0 rests in u (its down-leg wrote tmp); a coarser patch level ends in tmp (its up-leg
      // cannot run in place)
      Q.up = LEG_PATCH;
      Q.prolong = PROLONG_LOADING;
      Q.rests_tmp = l >= 1;
    } else if (jacobi_fuses_prolong(s, l)) {
      Q.up = LEG_PLAIN;
      Q.prolong = PROLONG_OWN_SMOOTHER;
    } else {
      Q.prolong = fuses_jacobi_prolong(s, l) ? PROLONG_COARSER_SWEEP
                                             : (l == lp && solve_prolongs) ? PROLONG_SOLVE : PROLONG_TRANSFER;
      if (l >= 2 && duo[(size_t)l] == l - 1) {
        // the finer level's up-leg reads the halo of u that other tiles own: it ends in tmp
        Q.up = LEG_DUO_COARSE;
        LevelPlan& F = P.lv[(size_t)--l];
        F.up = LEG_DUO_FINE;
        F.prolong = PROLONG_COARSER_SWEEP;
        F.rests_tmp = true;
      } else {
        Q.up = pair_up_ok(s, l) ? LEG_PAIR : LEG_PLAIN;
      }
    }
  }
  // K-March: the plain legs that sweep from phase 0 and prolong nowhere
  for (int l = 0; march_cycle && l < nl; ++l) {
    LevelPlan& Q = P.lv[(size_t)l];
    MarchRef R;
    if (!march_fill(s, l, level_vecs(s->lv[l], false), &R)) continue;
    Q.march_down = Q.down == LEG_PLAIN && Q.phase == 0;
    Q.march_up = Q.up == LEG_PLAIN && Q.prolong != PROLONG_OWN_SMOOTHER &&
                 !(l >= 1 && P.lv[(size_t)l - 1].prolong == PROLONG_COARSER_SWEEP);
  }
  return P;
}
// the plan the accessors answer from: of the cycle enqueued last, before the first one of the cycle
// that would run
CyclePlan current_plan(const amg_hip_solver* s) {
  return s->plan_kept ? s->plan : build_cycle_plan(s, CYCLE_ALL, SEAM_OFF);
}
// Where a level's iterate lives, by the plan.  Between cycles (the accessors, the level operations):
LevelVecs resting(amg_hip_solver* s, const CyclePlan& P, int l) {
  return level_vecs(s->lv[l], P.lv[(size_t)l].rests_tmp);
}
// ... between its two legs (before its down-leg every level has it in u) ...
LevelVecs between_legs(amg_hip_solver* s, const CyclePlan& P, int l) {
  return level_vecs(s->lv[l], P.lv[(size_t)l].march_down);
}
// ... and after its up-leg (the finer level's prolongation reads it): where it rests, or tmp until the copy home.
// (Only K-Patch and K-Duo launches read a level that rests in tmp; under a multicolour, own-smoother or transfer
// prolongation the plan never puts one, so those read the level's u as ever.)
double* after_up(amg_hip_solver* s, const CyclePlan& P, int l) {
  return level_vecs(s->lv[l], P.lv[(size_t)l].rests_tmp || P.lv[(size_t)l].home_copy()).u;
}
// where the prolongation INTO level l lands: a level whose two post-sweeps run as one launch reads
// u + P u_{l+1} from tmp (its second sweep then writes u; no in-place race between the tiles),
// every other level takes it in place
double* up_target(amg_hip_solver* s, const CyclePlan& P, int l) {
  const LevelVecs v = between_legs(s, P, l);
  return P.lv[(size_t)l].up_tmp ? v.tmp : v.u;
}

// one symmetric pass: colours 0..nc-1 then nc-1..0; a colour that directly follows itself is not
// launched again (mc_sequence: the repeat would store the bits already there).  again: the pass
// follows another pass of the same smoothing call (its colour 0 directly follows colour 0).
amg_hip_status enqueue_multicolor(StepCtx& X, amg_hip_solver* s, Level& L, double* u, bool again) {
  hipStream_t st = X.st;
  const DevMat& A = L.mc_mat;
  if (L.mc_dict && L.mc_start_dev.p && !s->opt.no_fusion) {  // small level: the whole pass in one launch
    // every row twice: code words 8 B per word and row + 4 B dof id, f, u written
    X.count(2.0 * ((8.0 * L.mc_words + 4.0) * L.n + 16.0 * L.n));
    HIP_TRY(launch_dict_gs_sweep(L.n_colors, L.mc_start_dev.as<int32_t>(), L.mc_start.back(), L.mc_words,
                                 L.mc_wmax, L.mc_codes.as<uint64_t>(), L.mc_rowid.as<int32_t>(),
                                 L.mc_doff.as<int32_t>(), L.mc_dval.as<double>(), L.mc_ntab,
                                 L.f.as<double>(), u, st));
    return AMG_HIP_OK;
  }
  // per row of a launched colour: matrix stream (dictionary: code words + 4 B dof id; SELL panels:
  // indices + values + 4 B dof id), f, u written
  const double row_bytes = (L.mc_dict ? 8.0 * L.mc_words + 4.0 : (mat_bytes(A) + 4.0 * L.n) / (double)std::max<int64_t>(L.n, 1)) + 16.0;
  auto one = [&](int c) -> hipError_t {
    X.count(row_bytes * (double)(L.mc_start[c + 1] - L.mc_start[c]));
    if (L.mc_dict)
      return launch_dict_gs_color(L.mc_start[c], L.mc_start[c + 1] - L.mc_start[c], L.mc_words,
                                  L.mc_wmax, L.mc_codes.as<uint64_t>(), L.mc_rowid.as<int32_t>(),
                                  L.mc_doff.as<int32_t>(), L.mc_dval.as<double>(), L.mc_ntab,
                                  L.f.as<double>(), u, st);
    return launch_sell_gs_color(A.n_rows, A.max_width, A.soff.as<int64_t>(), A.scol.as<int32_t>(),
                                A.sval.as<double>(), L.mc_rowid.as<int32_t>(), L.mc_start[c],
                                L.mc_start[c + 1] - L.mc_start[c], L.f.as<double>(),
                                u, st);
  };
  const bool dedupe = !s->opt.no_fusion;
  for (int c = (again && dedupe) ? 1 : 0; c < L.n_colors; ++c) HIP_TRY(one(c));
  for (int c = L.n_colors - (dedupe ? 2 : 1); c >= 0; --c) HIP_TRY(one(c));
  return AMG_HIP_OK;
}

amg_hip_status enqueue_residual(StepCtx& X, amg_hip_solver* s, int l, const double* u) {
  Level& L = s->lv[l];
  HIP_TRY(launch_mat(CSR_RESID, L.A_rows, u, L.f.as<double>(), L.r.as<double>(), 1.0, X.st));
  X.count(mat_bytes(L.A_rows) + 24.0 * L.n);  // matrix, f, u, r
  return AMG_HIP_OK;
}

// roctx ranges per level and leg, AMG_HIP_ROCTX=1: "L<l> down" / "L<l> up" /
// "coarse solve" around what is ENQUEUED for them (librocprofiler-sdk-roctx by dlopen; the ranges
// bracket the launches, so they line up with the kernels in a `rocprofv3 --marker-trace
// --kernel-trace` run of an eager cycle, use_graph = 0 / bench.py --no-graph; under a captured
// graph they mark the capture only).
struct Roctx {
  int (*push)(const char*) = nullptr;
  int (*pop)() = nullptr;
  Roctx() {
    if (!std::getenv("AMG_HIP_ROCTX")) return;
    void* h = dlopen("librocprofiler-sdk-roctx.so", RTLD_NOW | RTLD_LOCAL);
    if (!h) h = dlopen("libroctx64.so", RTLD_NOW | RTLD_LOCAL);
    if (!h) return;
    push = (int (*)(const char*))dlsym(h, "roctxRangePushA");
    pop = (int (*)())dlsym(h, "roctxRangePop");
    if (!push || !pop) push = nullptr;
  }
};
struct RoctxRange {
  static Roctx& api() {
    static Roctx r;
    return r;
  }
  bool on = false;
  RoctxRange(const char* what, int level) {
    if (!api().push) return;
    char name[48];
    if (level >= 0) std::snprintf(name, sizeof(name), "L%d %s", level, what);
    else std::snprintf(name, sizeof(name), "%s", what);
    api().push(name);
    on = true;
  }
  ~RoctxRange() {
    if (on) api().pop();
  }
};

// What the double cycle enqueues on: the stream and the bytes its launches have to move (StepCtx, all
// of them in `once`), the part, and the piece of the seam sequence (SEAM_*) with the level-0 buffer it
// hands over in (0: tmp, 1: r).  Part and piece choose which levels the enqueue walks.
struct CycleCtx : StepCtx {
  int part = CYCLE_ALL, piece = SEAM_OFF, src = 0;
};
// ---- the unfused transfers: linear, tensor, axis or CSR ----------------------------------------
// f_{l+1} = R r_l (:281-282).  uH (zero_coarse_u): also u_{l+1} = 0 there (:278) -- when the smoother starts
// from "u == 0" without reading u, the fill itself is dead (u_{l+1} is fully overwritten before
// anyone reads it)
amg_hip_status enqueue_restrict(StepCtx& X, amg_hip_solver* s, int l, double* uH) {
  Level& L = s->lv[l];
  Level& C = s->lv[l + 1];
  hipStream_t st = X.st;
  const bool zero_coarse_u = uH != nullptr;
  if (L.linear && s->opt.stencil_transfers) {
    HIP_TRY(launch_linear_restrict(L.n, C.n, L.r.as<double>(), C.f.as<double>(), uH, st));
    X.count(8.0 * L.n + (zero_coarse_u ? 16.0 : 8.0) * C.n);
  } else if (L.tensor_stencil) {                               // the same two steps, full coarsening
    HIP_TRY(launch_tensor_restrict(L.tdim, L.dims, L.tmask, L.tsides, L.tper, L.r.as<double>(), C.f.as<double>(), uH, st));
    X.count(8.0 * L.n + (zero_coarse_u ? 16.0 : 8.0) * C.n);
  } else if (L.axis_stencil) {                                 // the same two steps, one axis, weights of A_l
    HIP_TRY(launch_axis_restrict(L.tdim, L.dims, L.axis, L.axis_periodic(), L.axis_W_dev.as<double>(), L.r.as<double>(),
                                 C.f.as<double>(), uH, st));
    X.count(8.0 * L.n + 16.0 * (L.n - C.n) + (zero_coarse_u ? 16.0 : 8.0) * C.n);
  } else {
    if (zero_coarse_u) HIP_TRY(hipMemsetAsync(uH, 0, sizeof(double) * C.n, st));  // :278
    const DevCsr& R = L.R_rows;
    HIP_TRY(launch_csr(CSR_SPMV, R.n_rows, R.nnz, R.max_block_nnz, R.max_row_nnz,
                       R.rowptr(), R.col(), R.v(), L.r.as<double>(), nullptr,
                       C.f.as<double>(), 1.0, 0, st));
    X.count(12.0 * R.nnz + 4.0 * C.n + 8.0 * L.n + (zero_coarse_u ? 16.0 : 8.0) * C.n);
  }
  return AMG_HIP_OK;
}
// out = u + P uH (:294-296), u and uH the iterates of levels l and l+1; out is u itself, or (linear
// transfers only) the level's other buffer
amg_hip_status enqueue_prolong_add(StepCtx& X, amg_hip_solver* s, int l, const double* uH, double* u, double* out) {
  Level& L = s->lv[l];
  Level& C = s->lv[l + 1];
  hipStream_t st = X.st;
  if (L.linear && s->opt.stencil_transfers) {
    if (out != u)
      HIP_TRY(launch_linear_prolong_to(L.n, C.n, uH, u, out, st));
    else
      HIP_TRY(launch_linear_prolong_add(L.n, C.n, uH, u, st));
    X.count(8.0 * C.n + 16.0 * L.n);
  } else if (L.tensor_stencil) {
    HIP_TRY(launch_tensor_prolong_add(L.tdim, L.dims, L.tmask, L.tsides, L.tper, uH, u, st));
    X.count(8.0 * C.n + 16.0 * L.n);
  } else if (L.axis_stencil) {
    HIP_TRY(launch_axis_prolong_add(L.tdim, L.dims, L.axis, L.axis_periodic(), L.axis_W_dev.as<double>(), uH, u, st));
    X.count(16.0 * L.n + 16.0 * (L.n - C.n) + 8.0 * C.n);
  } else {
    const DevCsr& P = L.P_rows;  // u_h = u_h + P u_H in one launch
    HIP_TRY(launch_csr(CSR_SPMV_ADD, P.n_rows, P.nnz, P.max_block_nnz, P.max_row_nnz,
                       P.rowptr(), P.col(), P.v(), uH, u, u, 1.0, 0, st));
    X.count(12.0 * P.nnz + 4.0 * L.n + 8.0 * C.n + 16.0 * L.n);
  }
  return AMG_HIP_OK;
}

// ---- one function per launch form and leg (multigrid.hpp:263-305) ------------------------------
// share of a level's lines a ranged (slab, window) K-Patch launch covers
double patch_range_frac(const Level& L, bool ranged, int64_t lo, int64_t hi) {
  if (!ranged || hi < 0) return 1.0;
  const double lines = (double)((L.n + L.A_rows.patch_m - 1) / L.A_rows.patch_m);
  return std::min(1.0, (double)(hi - lo) / lines);
}
// :268 (the colour stages of the symmetric passes) + :272-282
amg_hip_status down_mc_patch(CycleCtx& X, amg_hip_solver* s, int l) {
  Level& L = s->lv[l];
  Level& C = s->lv[l + 1];
  const DevMat& A = L.A_rows;
  int nd = 0;
  const std::vector<McLaunch> plan = mc_plan(s, l, &nd);
  for (int q = 0; q < nd; ++q) {
    const McLaunch& M = plan[(size_t)q];
    HIP_TRY(launch_patch_rb(false, M.tail, L.n, A.patch_m, A.patch_ref(), M.in, L.f.as<double>(), nullptr, C.n,
                            M.out, (M.tail && s->opt.keep_residual) ? L.r.as<double>() : nullptr,
                            M.tail ? C.f.as<double>() : nullptr, M.tail ? C.u.as<double>() : nullptr, M.stages,
                            (uint32_t)L.mc_ctab, X.st));
  }
  // each launch: row types + x + f + out; the last also f_H, zeroed u_H (and r when kept)
  X.count(nd * 25.0 * L.n + 16.0 * C.n + (s->opt.keep_residual ? 8.0 * L.n : 0.0));
  return AMG_HIP_OK;
}
// :294-296 + :300 (the colour stages of the symmetric passes)
amg_hip_status up_mc_patch(CycleCtx& X, amg_hip_solver* s, const CyclePlan& P, int l) {
  Level& L = s->lv[l];
  Level& C = s->lv[l + 1];
  const DevMat& A = L.A_rows;
  int nd = 0;
  const std::vector<McLaunch> plan = mc_plan(s, l, &nd);
  for (size_t q = (size_t)nd; q < plan.size(); ++q) {
    const McLaunch& M = plan[q];
    HIP_TRY(launch_patch_rb(M.prolong, false, L.n, A.patch_m, A.patch_ref(), M.in, L.f.as<double>(),
                            M.prolong ? after_up(s, P, l + 1) : nullptr, C.n, M.out, nullptr, nullptr, nullptr,
                            M.stages, (uint32_t)L.mc_ctab, X.st));
  }
  X.count((double)(plan.size() - (size_t)nd) * 25.0 * L.n + 8.0 * C.n);
  return AMG_HIP_OK;
}
// :268 + :272-282 of a narrow level, one launch: u -> tmp
amg_hip_status down_mc_strip(CycleCtx& X, amg_hip_solver* s, int l) {
  Level& L = s->lv[l];
  Level& C = s->lv[l + 1];
  StripRef R = mc_strip_ref(s, l);
  R.x = L.u.as<double>();
  R.u_out = L.tmp.as<double>();
  R.r_out = s->opt.keep_residual ? L.r.as<double>() : nullptr;
  R.fH = C.f.as<double>();
  R.uH_zero = C.u.as<double>();
  HIP_TRY(launch_mc_strip(false, true, R, L.A_rows.dict_ref(), X.st));
  // row types + colours + x + f + out; f_H, zeroed u_H (and r when kept)
  X.count(26.0 * L.n + 16.0 * C.n + (s->opt.keep_residual ? 8.0 * L.n : 0.0));
  return AMG_HIP_OK;
}
// :294-296 + :300 of a narrow level, one launch: tmp + P u_H -> u
amg_hip_status up_mc_strip(CycleCtx& X, amg_hip_solver* s, const CyclePlan& P, int l) {
  Level& L = s->lv[l];
  Level& C = s->lv[l + 1];
  StripRef R = mc_strip_ref(s, l);
  R.x = L.tmp.as<double>();
  R.u_out = L.u.as<double>();
  R.uH = after_up(s, P, l + 1);
  HIP_TRY(launch_mc_strip(true, false, R, L.A_rows.dict_ref(), X.st));
  X.count(26.0 * L.n + 8.0 * C.n);
  return AMG_HIP_OK;
}
// :268 (both sweeps) + :272-282 + :268 of l+1, one launch
amg_hip_status down_patch(CycleCtx& X, amg_hip_solver* s, const CyclePlan& P, int l) {
  Level& L = s->lv[l];
  Level& C = s->lv[l + 1];
  const DevMat& A = L.A_rows;
  hipStream_t st = X.st;
  if (l == 0 && X.piece == SEAM_CYCLE) {  // up-leg of the last cycle + this down-leg: one launch
    HIP_TRY(launch_patch_seam(L.n, A.patch_m, A.patch_ref(5), seam_buf(s, X.src), L.f.as<double>(),
                              C.tmp.as<double>(), C.n, seam_buf(s, 1 - X.src), C.f.as<double>(),
                              s->opt.omega, st));
    X.count(25.0 * L.n + 16.0 * C.n);  // row types + x + f + smoothed u; u_H, f_H
    return AMG_HIP_OK;
  }
  const Slab& sb = s->slab;
  const bool ranged = X.part == CYCLE_SLAB_DOWN;
  const bool first = l == 0;  // l >= 1: the first sweep came from level l-1's kernel (in tmp) ...
  const bool xf_in = P.lv[(size_t)l].xf_in;    // ... or is formed from f here
  const bool xf_out = P.lv[(size_t)l].xf_out;  // level l+1 forms its own: f_H only
  HIP_TRY(launch_patch_down(first, L.n, A.patch_m, A.patch_ref(patch_rings(s, first)),
                            first ? L.u.as<double>() : (xf_in ? nullptr : L.tmp.as<double>()),
                            L.f.as<double>(),
                            first ? (X.piece == SEAM_HEAD ? seam_buf(s, X.src) : L.tmp.as<double>())
                                  : L.u.as<double>(),
                            s->opt.keep_residual ? L.r.as<double>() : nullptr, C.n,
                            C.f.as<double>(), C.diag.as<double>(), xf_out ? nullptr : C.tmp.as<double>(),
                            s->opt.omega, st, ranged ? sb.down_lo[l] : 0,
                            ranged ? sb.down_hi[l] : -1, xf_in));
  // row types + [x +] f + smoothed u; f_H [, first coarse sweep, coarse diagonal]
  // (the coarse diagonal is not read under the tiles that take it as an argument)
  X.count(patch_range_frac(L, ranged, ranged ? sb.down_lo[l] : 0, ranged ? sb.down_hi[l] : -1) *
          ((xf_in ? 17.0 : 25.0) * L.n + (xf_out ? 8.0 : 24.0 - 8.0 * A.patch_cfrac) * C.n +
           (s->opt.keep_residual ? 8.0 * L.n : 0.0)));
  return AMG_HIP_OK;
}
// :294-296 + :300 (both sweeps), one launch
amg_hip_status up_patch(CycleCtx& X, amg_hip_solver* s, const CyclePlan& P, int l) {
  Level& L = s->lv[l];
  Level& C = s->lv[l + 1];
  const DevMat& A = L.A_rows;
  const Slab& sb = s->slab;
  const bool ranged = X.part == CYCLE_SLAB_UP;
  const bool top = l == 0;  // level 0 rests in u (its down-leg wrote tmp); coarser patch levels end in tmp
  HIP_TRY(launch_patch_up(L.n, A.patch_m, A.patch_ref(patch_rings(s, false)),
                          top ? L.tmp.as<double>() : L.u.as<double>(), L.f.as<double>(),
                          after_up(s, P, l + 1), C.n,
                          top ? L.u.as<double>() : L.tmp.as<double>(), s->opt.omega, X.st,
                          ranged ? sb.up_lo[l] : 0, ranged ? sb.up_hi[l] : -1));
  // row types + x + f + out; u_H
  X.count(patch_range_frac(L, ranged, ranged ? sb.up_lo[l] : 0, ranged ? sb.up_hi[l] : -1) * (25.0 * L.n + 8.0 * C.n));
  return AMG_HIP_OK;
}
// K-Tail: levels l .. L-2, the solve and the way back: ONE launch
amg_hip_status enqueue_tail(CycleCtx& X, amg_hip_solver* s, const CyclePlan& P, int l) {
  const int nl = (int)s->lv.size();
  TailRef T;
  std::memset(&T, 0, sizeof(T));
  T.nlev = nl - 1 - l;
  for (int q = 0; q < T.nlev; ++q) {
    Level& Q = s->lv[l + q];
    const DictRef D = Q.A_rows.dict_ref();
    TailLevelRef& R = T.L[q];
    R.n = (int)Q.n;
    R.hbw = (Q.A_rows.dict_hb + 1) & ~1;
    R.words = D.words;
    R.ntab = D.ntab;
    R.rtype = D.rtype;
    R.rwords = D.rwords;
    R.doff = D.doff;
    R.dval = D.dval;
    R.f = Q.f.as<double>();
    R.u = Q.u.as<double>();
    R.tmp = Q.tmp.as<double>();
    R.diag = Q.diag.as<double>();
  }
  Level& C = s->lv[nl - 1];
  T.nc = (int)C.n;
  T.wc = (int)s->coarse.w;
  T.cf = s->coarse.sf.as<double>();
  T.cb = s->coarse.sb.as<double>();
  T.dg = s->coarse.d.as<double>();
  T.fc = C.f.as<double>();
  T.uc = C.u.as<double>();
  T.tmpc = C.tmp.as<double>();
  T.diagc = C.diag.as<double>();
  Level& F = s->lv[l - 1];
  T.n_fine = (int)F.n;
  T.uf_in = between_legs(s, P, l - 1).u;
  T.uf_out = up_target(s, P, l - 1);
  T.omega = s->opt.omega;
  HIP_TRY(launch_tail(T, X.st));
  for (int q = 0; q < T.nlev; ++q) {  // what the pair kernels of these levels would have moved
    const Level& Q = s->lv[l + q];
    const double nH = (double)s->lv[l + q + 1].n, nF = (double)s->lv[l + q - 1].n;
    X.count(2.0 * (mat_bytes(Q.A_rows) + 24.0 * Q.n) + 24.0 * nH + 16.0 * nF);
  }
  X.count(16.0 * (double)C.n * (double)std::max<int64_t>(s->coarse.w, 1) + 24.0 * C.n);
  return AMG_HIP_OK;
}
// K-Duo, down: the pair launches of levels l and l+1 in one
amg_hip_status down_duo(CycleCtx& X, amg_hip_solver* s, int l) {
  Level& L = s->lv[l];
  Level& C = s->lv[l + 1];
  Level& CC = s->lv[l + 2];
  const DevMat& A = L.A_rows;
  const DevMat& AC = C.A_rows;
  const bool keep = s->opt.keep_residual != 0;
  HIP_TRY(launch_dict_duo_down(A.n_rows, A.dict_ref(), A.dict_hb, AC.n_rows, AC.dict_ref(), AC.dict_hb,
                               L.tmp.as<double>(), L.f.as<double>(), L.u.as<double>(),
                               keep ? L.r.as<double>() : nullptr, C.f.as<double>(), C.diag.as<double>(),
                               C.u.as<double>(), keep ? C.r.as<double>() : nullptr, CC.n, CC.f.as<double>(),
                               CC.diag.as<double>(), CC.tmp.as<double>(), s->opt.omega, X.st));
  // what the pair launches of the two levels would have moved
  X.count(mat_bytes(A) + 24.0 * L.n + 24.0 * C.n + (keep ? 8.0 * L.n : 0.0));
  X.count(mat_bytes(AC) + 24.0 * C.n + 24.0 * CC.n + (keep ? 8.0 * C.n : 0.0));
  return AMG_HIP_OK;
}
// K-Duo, up (l: the coarser level): :300 of levels l and l-1 and the prolongations between and after
// them in one launch; level l-1 ends in tmp
amg_hip_status up_duo(CycleCtx& X, amg_hip_solver* s, const CyclePlan& P, int l) {
  Level& L = s->lv[l];
  Level& F = s->lv[l - 1];
  Level& FF = s->lv[l - 2];
  const DevMat& A = L.A_cols();
  const DevMat& AF = F.A_cols();
  HIP_TRY(launch_dict_duo_up(AF.n_rows, AF.dict_ref(), AF.dict_hb, A.n_rows, A.dict_ref(), A.dict_hb,
                             L.tmp.as<double>(), L.f.as<double>(), L.u.as<double>(), F.u.as<double>(),
                             F.f.as<double>(), F.tmp.as<double>(), s->opt.omega, FF.n, between_legs(s, P, l - 2).u,
                             up_target(s, P, l - 2), X.st));
  // what the pair launches of the two levels would have moved
  X.count(mat_bytes(A) + 24.0 * L.n + 16.0 * F.n);
  X.count(mat_bytes(AF) + 24.0 * F.n + 16.0 * FF.n);
  return AMG_HIP_OK;
}
// second pre-sweep + residual + restriction + :268 of l+1
amg_hip_status down_pair(CycleCtx& X, amg_hip_solver* s, int l) {
  Level& L = s->lv[l];
  Level& C = s->lv[l + 1];
  const DevMat& A = L.A_rows;
  HIP_TRY(launch_dict_pair_down(A.n_rows, A.dict_ref(), A.dict_hb, L.tmp.as<double>(),
                                L.f.as<double>(), L.u.as<double>(),
                                s->opt.keep_residual ? L.r.as<double>() : nullptr, C.n,
                                C.f.as<double>(), C.diag.as<double>(), C.tmp.as<double>(),
                                s->opt.omega, X.st));
  X.count(mat_bytes(A) + 24.0 * L.n + 24.0 * C.n + (s->opt.keep_residual ? 8.0 * L.n : 0.0));
  return AMG_HIP_OK;
}
// :300, both sweeps; the second prolongs into level l-1
amg_hip_status up_pair(CycleCtx& X, amg_hip_solver* s, const CyclePlan& P, int l) {
  Level& L = s->lv[l];
  Level& F = s->lv[l - 1];
  const DevMat& A = L.A_cols();
  HIP_TRY(launch_dict_pair_up(A.n_rows, A.dict_ref(), A.dict_hb, L.tmp.as<double>(),
                              L.f.as<double>(), L.u.as<double>(), s->opt.omega, F.n,
                              between_legs(s, P, l - 1).u, up_target(s, P, l - 1), X.st));
  X.count(mat_bytes(A) + 24.0 * L.n + 16.0 * F.n);
  return AMG_HIP_OK;
}
// :268, then :272-282 (+ :268 of l+1 when fused)
amg_hip_status down_plain(CycleCtx& X, amg_hip_solver* s, const CyclePlan& P, int l) {
  const LevelPlan& Q = P.lv[(size_t)l];
  AMG_TRY(enqueue_smooth(X, s, l, level_vecs(s->lv[l], false), Sweep{Q.phase, Q.march_down}));  // :268
  const double* u = between_legs(s, P, l).u;
  if (Q.restrict_fused) {                                                // :272-282 + :268 of l+1
    Level& L = s->lv[l];
    Level& C = s->lv[l + 1];
    const DevMat& A = L.A_rows;
    const bool zero_known = P.zero_known;
    HIP_TRY(launch_dict_resid_restrict(A.n_rows, A.dict_ref(), u,
                                       L.f.as<double>(),
                                       s->opt.keep_residual ? L.r.as<double>() : nullptr, C.n,
                                       C.f.as<double>(),
                                       zero_known ? C.diag.as<double>() : nullptr,
                                       zero_known ? C.tmp.as<double>() : nullptr,
                                       C.u.as<double>(), s->opt.omega, X.st));
    // matrix, u, f (r when kept); f_H and either the first coarse sweep + diagonal or the zeroed u_H
    X.count(mat_bytes(A) + 16.0 * L.n + (s->opt.keep_residual ? 8.0 * L.n : 0.0) +
            (zero_known ? 24.0 : 16.0) * C.n);
    return AMG_HIP_OK;
  }
  AMG_TRY(enqueue_residual(X, s, l, u));                                 // :272-274
  if (l + 1 != (int)s->lv.size())                                        // :278 + :281-282
    AMG_TRY(enqueue_restrict(X, s, l, P.zero_known ? nullptr : s->lv[l + 1].u.as<double>()));
  return AMG_HIP_OK;
}
// :300; the last sweep also prolongs into level l-1 when that fuses
amg_hip_status up_plain(CycleCtx& X, amg_hip_solver* s, const CyclePlan& P, int l) {
  const LevelPlan& Q = P.lv[(size_t)l];
  Sweep w{Q.prolong == PROLONG_OWN_SMOOTHER ? 2 : 0, Q.march_up};  // 2: :294-296 inside :300
  w.coarse_u = after_up(s, P, l + 1);
  if (l >= 1 && P.lv[(size_t)l - 1].prolong == PROLONG_COARSER_SWEEP) {
    w.fine_u = between_legs(s, P, l - 1).u;
    w.fine_out = up_target(s, P, l - 1);
  }
  w.reverse = w.phase == 0;
  return enqueue_smooth(X, s, l, between_legs(s, P, l), w);
}

// multigrid.hpp:263-305: two loops that dispatch on the plan.  The slab and window ranges (X.part) and
// the seam pieces (X.piece) choose which levels it walks.
amg_hip_status enqueue_vcycle_body(CycleCtx& X, amg_hip_solver* s) {
  const int nl = (int)s->lv.size();
  hipStream_t st = X.st;
  const int k = s->slab.levels;
  const int part = X.part;
  const bool ranged = part == CYCLE_SLAB_DOWN || part == CYCLE_SLAB_UP;
  const CyclePlan P = build_cycle_plan(s, part, X.piece);
  if (!ranged) {
    s->plan = P;
    s->plan_kept = true;
  }
  if (part == CYCLE_SLAB_TAIL && !P.lv[(size_t)k - 1].xf_out) {  // (a K-Patch level below the cut forms that sweep itself)
    Level& L = s->lv[k];
    HIP_TRY(launch_jacobi_from_zero(L.n, L.diag.as<double>(), L.f.as<double>(), L.tmp.as<double>(),
                                    s->opt.omega, st));
    X.count(24.0 * L.n);
  }
  // the seam sequence (part == CYCLE_ALL): head = the cycle without the level-0 up-leg, its level-0
  // down-leg writing seam_buf(src); seam cycle = the seam launch from seam_buf(src) into the other
  // buffer, then levels 1 .. L-1 as in the cycle; finish = the level-0 up-leg alone, from tmp
  const int piece = X.piece;
  const int down_from = part == CYCLE_SLAB_TAIL ? k : 0;
  const int down_to = part == CYCLE_SLAB_DOWN ? k : ((part == CYCLE_SLAB_UP || piece == SEAM_FINISH) ? 0 : nl);
  for (int l = down_from; l < down_to; ++l) {
    const LegForm form = P.lv[(size_t)l].down;
    if (form == LEG_NONE || form == LEG_IN_TAIL || form == LEG_DUO_COARSE) continue;  // no launch of its own
    RoctxRange range("down", l);
    switch (form) {
      case LEG_MC_PATCH: AMG_TRY(down_mc_patch(X, s, l)); break;
      case LEG_MC_STRIP: AMG_TRY(down_mc_strip(X, s, l)); break;
      case LEG_PATCH: AMG_TRY(down_patch(X, s, P, l)); break;
      case LEG_TAIL_HEAD: AMG_TRY(enqueue_tail(X, s, P, l)); break;
      case LEG_DUO_FINE: AMG_TRY(down_duo(X, s, l)); break;
      case LEG_PAIR: AMG_TRY(down_pair(X, s, l)); break;
      default: AMG_TRY(down_plain(X, s, P, l)); break;
    }
  }
  const bool tail_done = P.tail_first >= 0 && down_to == nl;
  if (!ranged && !tail_done && piece != SEAM_FINISH) {             // :287-288
    RoctxRange range("coarse solve", -1);
    if (s->opt.window)
      return fail(AMG_HIP_EINVAL, "a window solver (opt.window) runs by parts: amg_hip_window_run");
    Level& C = s->lv[nl - 1];
    const LevelVecs vc = between_legs(s, P, nl - 1);
    const int lp = nl - 2;  // plain stencil prolongation into level L-2: one launch less when fused
    if (lp >= 0 && P.lv[(size_t)lp].prolong == PROLONG_SOLVE) {
      Level& Lp = s->lv[lp];
      HIP_TRY(launch_coarse(s->coarse, C.f.as<double>(), vc.tmp, vc.u, st, Lp.n, between_legs(s, P, lp).u,
                            up_target(s, P, lp)));
      X.count(16.0 * Lp.n);
    } else {
      HIP_TRY(launch_coarse(s->coarse, C.f.as<double>(), vc.tmp, vc.u, st));
    }
    // banded L D L^T solve: the band of L forwards and backwards, D, f, u
    X.count(16.0 * (double)C.n * (double)std::max<int64_t>(s->coarse.w, 1) + 24.0 * C.n);
  }
  const int up_from = piece == SEAM_FINISH ? 0 : (part == CYCLE_SLAB_UP ? k - 1 : (part == CYCLE_SLAB_DOWN ? -1 : (tail_done ? P.tail_first - 1 : nl - 2)));
  const int up_to = part == CYCLE_SLAB_TAIL ? k : ((piece == SEAM_HEAD || piece == SEAM_CYCLE) ? 1 : 0);
  for (int l = up_from; l >= up_to; --l) {                         // :291
    const LevelPlan& Q = P.lv[(size_t)l];
    if (Q.up == LEG_DUO_FINE) continue;  // done by the launch of level l+1
    RoctxRange range("up", l);
    if (Q.prolong == PROLONG_TRANSFER)                             // :294-296
      AMG_TRY(enqueue_prolong_add(X, s, l, after_up(s, P, l + 1), between_legs(s, P, l).u, up_target(s, P, l)));
    switch (Q.up) {
      case LEG_MC_PATCH: AMG_TRY(up_mc_patch(X, s, P, l)); break;
      case LEG_MC_STRIP: AMG_TRY(up_mc_strip(X, s, P, l)); break;
      case LEG_PATCH: AMG_TRY(up_patch(X, s, P, l)); break;
      case LEG_DUO_COARSE: AMG_TRY(up_duo(X, s, P, l)); break;
      case LEG_PAIR: AMG_TRY(up_pair(X, s, P, l)); break;
      default: AMG_TRY(up_plain(X, s, P, l)); break;
    }
  }
  // a level K-March swept on one leg only ends the cycle with its solution in tmp: it goes home
  for (int l = 0; l < nl; ++l) {
    const Level& L = s->lv[l];
    if (!P.lv[(size_t)l].home_copy()) continue;
    HIP_TRY(hipMemcpyAsync(L.u.p, L.tmp.p, sizeof(double) * L.n, hipMemcpyDeviceToDevice, st));
    X.count(16.0 * L.n);
  }
  return AMG_HIP_OK;
}
// the cycle (or part, or seam piece) on the solver's stream; its bytes go to must_move when it is enqueued
amg_hip_status enqueue_vcycle(amg_hip_solver* s, int part = CYCLE_ALL, int piece = SEAM_OFF, int src = 0) {
  CycleCtx X{{s->stream}, part, piece, src};
  const amg_hip_status r = enqueue_vcycle_body(X, s);
  // (the pieces of the seam sequence count apart: [0] stays the stand-alone cycle)
  s->must_move[piece == SEAM_CYCLE ? 4 : (piece != SEAM_OFF ? 5 : part)] = X.once;
  return r;
}

// One piece of the seam sequence (SEAM_HEAD / SEAM_CYCLE with the buffer src it hands over in, or
// SEAM_FINISH), enqueued or replayed from its graph, captured on first use.
amg_hip_status run_seam(amg_hip_solver* s, int piece, int src) {
  const int gi = piece == SEAM_FINISH ? 4 : (piece == SEAM_HEAD ? 0 : 2) + src;
  return replay_or_enqueue(s->opt.use_graph, s->seam_graph[gi], s->stream,
                           [s, piece, src] { return enqueue_vcycle(s, CYCLE_ALL, piece, src); });
}

amg_hip_status set_device(const amg_hip_solver* s) {
  if (s->opt.host_only)
    return fail(AMG_HIP_EINVAL, "solver was created with host_only = 1: no device state");
  HIP_TRY(hipSetDevice(s->device));
  return AMG_HIP_OK;
}

// K-Patch down-legs: which tiles sit over coarse rows that all share one diagonal value (the
// interior of the coarse level) -- those workgroups take it as a kernel argument instead of loading
// it per coarse row at the end of their life.  Called once the whole hierarchy is on the device.
amg_hip_status set_patch_coarse_flags(amg_hip_solver* s) {
  for (size_t l = 0; l + 1 < s->lv.size(); ++l) {
    Level& L = s->lv[l];
    Level& C = s->lv[l + 1];
    DevMat& A = L.A_rows;
    if (!A.patch || !C.diag.p || C.n < 1) continue;
    // geometry of the level's down-leg (the colour launches run on three rings)
    const int rings = s->opt.smoother == AMG_HIP_SM_MULTICOLOR_GS ? 3 : patch_rings(s, l == 0);
    // reference value: the coarse row under the middle of the middle line (C.n / 2 would be a line end)
    const int64_t lines = (L.n + A.patch_m - 1) / A.patch_m;
    const int64_t cref = std::min<int64_t>(C.n - 1, ((lines / 2) * A.patch_m + A.patch_m / 2) >> 1);
    double dref = 0.0;
    HIP_TRY(hipMemcpy(&dref, C.diag.as<double>() + cref, sizeof(double), hipMemcpyDeviceToHost));
    // the 42-line tiling first: its share of set flags is what the bytes model quotes (patch_cfrac);
    // then, where the down-leg runs on other tiles, the flags of those
    for (int rg = 3; rg >= rings; --rg) {
      int64_t tiles = 0;
      HIP_TRY(launch_patch_tile_flags(L.n, A.patch_m, rg, nullptr, A.patch_ntypes, nullptr, &tiles, nullptr));
      HIP_TRY(A.patch_cflags.alloc(((size_t)tiles + 3) & ~(size_t)3));  // whole words, as the tile flags
      HIP_TRY(hipMemset(A.patch_cflags.p, 0, A.patch_cflags.bytes));
      HIP_TRY(launch_patch_coarse_flags(L.n, A.patch_m, rg, C.n, C.diag.as<double>(), dref,
                                        A.patch_cflags.as<uint8_t>(), nullptr));
      if (rg != 3) continue;
      std::vector<uint8_t> fl((size_t)tiles);
      HIP_TRY(hipMemcpy(fl.data(), A.patch_cflags.p, fl.size(), hipMemcpyDeviceToHost));
      int64_t on = 0;
      for (uint8_t f : fl) on += f != 0;
      A.patch_cfrac = g_patch_tile_flags && tiles > 0 ? (double)on / (double)tiles : 0.0;
    }
    A.patch_crings = rings;
    A.patch_dH = dref;
  }
  HIP_TRY(hipDeviceSynchronize());
  return AMG_HIP_OK;
}

// ---- bytes model ----------------------------------------------
void compute_bytes(amg_hip_solver* s) {
  const int nl = (int)s->lv.size();
  double total = 0;
  const int iters = s->opt.smoother_iters;
  int sweeps_per_smooth = iters;
  if (s->opt.smoother == AMG_HIP_SM_SPGS || s->opt.smoother == AMG_HIP_SM_MULTICOLOR_GS)
    sweeps_per_smooth = 2 * iters;
  if (s->opt.smoother == AMG_HIP_SM_CHEBYSHEV) sweeps_per_smooth = iters * s->opt.cheb_degree;
  for (int l = 0; l < nl; ++l) {
    const Level& L = s->lv[l];
    const double sweep = 12.0 * (double)L.nnz_struct + 28.0 * (double)L.n;
    if (l == 0) s->fine_sweep_bytes = sweep;
    // line smoother: every sweep is a residual plus the K-Line solve (80 B per row)
    double extra = s->opt.smoother == AMG_HIP_SM_LINE_JACOBI ? 80.0 * (double)L.n * sweeps_per_smooth : 0.0;
    // alternating line smoother: a residual plus a line solve per direction (K-LineX 64, K-Line 80 B per row)
    if (s->opt.smoother == AMG_HIP_SM_LINE_ALT) {
      const int nd = std::max(L.alt.n_dir, 1);
      sweeps_per_smooth = iters * nd;
      extra = 0.0;
      for (int d = 0; d < nd; ++d)
        extra += ((L.alt.n_dir > 0 && L.alt.axis[d] == 0 ? 64.0 : 80.0) * (double)L.n + L.alt.seam_bytes(d)) * iters;
    }
    // pre-smooth + residual on every level; post-smooth on all but the coarsest
    total += sweep * (sweeps_per_smooth + 1) + extra;
    if (l + 1 != nl) {
      total += sweep * sweeps_per_smooth + extra;
      const double nH = (double)s->lv[l + 1].n, nh = (double)L.n;
      total += 8.0 * nH;                                   // zero
      if (L.tensor_stencil) {                              // K-TensorRestrict / K-TensorProlong
        total += 8 * nh + 8 * nH;
        total += 16 * nh + 8 * nH;
        continue;
      }
      if (L.axis_stencil) {                                // K-AxisRestrict / K-AxisProlong: plus the weights
        total += 8 * nh + 16 * (nh - nH) + 8 * nH;
        total += 16 * nh + 16 * (nh - nH) + 8 * nH;
        continue;
      }
      double pnnz = 3.0;  // entries per column of P
      if (L.tensor) pnnz = ((L.tmask & 1u) ? 3.0 : 1.0) * ((L.tmask & 2u) ? 3.0 : 1.0) * ((L.tmask & 4u) ? 3.0 : 1.0);
      total += 12.0 * pnnz * nH + 4 * nH + 8 * nh + 8 * nH;   // restrict (CSR R)
      total += 12.0 * pnnz * nH + 4 * nh + 8 * nH + 16 * nh;  // prolong + add (CSR P)
    }
  }
  s->cycle_bytes = total;
}

// ---- setup --------------------------------------------------------------------
hipError_t device_dict_encode(const DevCsr& A, bool prune, int maxlen, DevMat* D, bool* ok);

// Semi-coarsening (amg_hip_create_tensor_semi): masks = the n_levels - 1 explicit axis masks, or
// null for the automatic rule (host_setup.hpp: tensor_auto_mask) with theta and min_coarse.
struct SemiRule {
  const int32_t* masks = nullptr;
  double theta = 0.5;
  int64_t min_coarse = 1;
  // amg_hip_create_tensor_opdep: one axis per level (the automatic rule is tensor_opdep_auto_mask,
  // theta is not used) and the weights of axis_opdep_P instead of tensor_P's
  bool opdep = false;
  const char* opdep_who = "amg_hip_create_tensor_opdep: ";  // the entry point a refused row is reported under
  // amg_hip_create_tensor_opdep_periodic(_dev): the spec's periodic axes are checked on top of the
  // rule and a coarsened periodic axis takes the seam form of axis_opdep_P; the _dev form builds on the
  // host unless amg_hip_set_periodic_device_setup(1) is in force (K-AxisWeights / K-AxisGalerkin PER)
  bool opdep_periodic = false;
};
// a one-level solver's coarsest right-hand side is the caller's b, which the pinned solve must not alter
const char* const SINGULAR_ONE_LEVEL =
    "`singular` = 1 needs a hierarchy of at least 2 levels: with one level the pinned solve would zero the last entry of "
    "the caller's own right-hand side";
// "" or what is wrong with opt.natural_sides / opt.singular; dim = 0: a constructor without level
// grids, which takes neither
// periodic (amg_hip_create_tensor_periodic, != 0): a periodic axis has no sides, and `singular` needs
// the sides of the other axes only
// per_ctor: the constructor is amg_hip_create_tensor_periodic or _periodic_dev (`cyclic_lines`)
std::string sides_error(const amg_hip_options& o, int dim, uint32_t periodic = 0, bool per_ctor = false) {
  if (o.cyclic_lines != 0 && o.cyclic_lines != 1)
    return "`cyclic_lines` must be 0 or 1, got " + std::to_string(o.cyclic_lines);
  if (o.cyclic_lines && !per_ctor)
    return "`cyclic_lines` = 1: only amg_hip_create_tensor_periodic and amg_hip_create_tensor_periodic_dev know "
           "the periodic axes of a grid; this constructor needs 0";
  if (o.cyclic_lines && o.smoother != AMG_HIP_SM_LINE_ALT)
    return "`cyclic_lines` = 1 needs the smoother AMG_HIP_SM_LINE_ALT (AMG_HIP_SM_LINE_JACOBI knows no grid "
           "lines and keeps open chains)";
  if (o.singular != 0 && o.singular != 1)
    return "`singular` must be 0 or 1, got " + std::to_string(o.singular);
  if (!dim) {
    if (o.natural_sides != 0)
      return "`natural_sides` = " + std::to_string(o.natural_sides) + ": only the tensor constructors (amg_hip_create_tensor, "
             "_tensor_semi, _tensor_dev, _tensor_semi_dev) know the sides of a grid; this constructor needs 0";
    if (o.singular)
      return "`singular` = 1 needs every side in `natural_sides`, which only the tensor constructors take";
    return "";
  }
  if (o.natural_sides < 0 || o.natural_sides >= (1 << (2 * dim)))
    return "`natural_sides` = " + std::to_string(o.natural_sides) + " has bits other than the " + std::to_string(2 * dim) +
           " sides of a " + std::to_string(dim) + "-D grid (bit 2a = low side of axis a, bit 2a + 1 = high side)";
  if (periodic) {
    int want = 0;
    for (int a = 0; a < dim; ++a) {
      if (!((periodic >> a) & 1u)) {
        want |= 3 << (2 * a);
      } else if ((o.natural_sides >> (2 * a)) & 3) {
        return "`natural_sides` = " + std::to_string(o.natural_sides) + " names a side of axis " +
               std::string(1, "xyz"[a]) + ", which `periodic_axes` = " + std::to_string(periodic) +
               " makes periodic: a periodic axis has no sides";
      }
    }
    if (o.singular && o.natural_sides != want)
      return "`singular` = 1 needs every side of the axes that are not periodic natural: `natural_sides` = " +
             std::to_string(want) + " with `periodic_axes` = " + std::to_string(periodic) + ", got " +
             std::to_string(o.natural_sides);
    return "";
  }
  if (o.singular && o.natural_sides != (1 << (2 * dim)) - 1)
    return "`singular` = 1 needs every side natural: `natural_sides` = " + std::to_string((1 << (2 * dim)) - 1) + ", got " +
           std::to_string(o.natural_sides);
  return "";
}
// "" or what is wrong with the axis mask of level l on the grid d
std::string semi_mask_error(int l, int dim, const int64_t d[3], int64_t mask) {
  const std::string at = "level " + std::to_string(l) + ": axis mask " + std::to_string(mask);
  if (mask == 0) return at + " coarsens no axis";
  if (mask < 0 || mask > 7) return at + " has bits other than 1 (x), 2 (y) and 4 (z)";
  if (dim == 2 && (mask & 4)) return at + " coarsens z, and `dim` is 2";
  for (int a = 0; a < 3; ++a)
    if (((mask >> a) & 1) && d[a] < 2)
      return at + " coarsens axis " + std::string(1, "xyz"[a]) + ", which has " + std::to_string(d[a]) +
             " point on this level (the grid is " + std::to_string(d[0]) + " x " + std::to_string(d[1]) + " x " +
             std::to_string(d[2]) + ")";
  return "";
}
// "" or what is wrong with `periodic_axes` itself
std::string periodic_axes_error(int dim, int64_t periodic) {
  if (periodic < 0 || periodic >= (1 << dim))
    return "`periodic_axes` = " + std::to_string(periodic) + " has bits other than the " + std::to_string(dim) +
           " axes of a " + std::to_string(dim) + "-D grid (bit a = axis a: 1 = x, 2 = y, 4 = z)";
  return "";
}
// "" or the periodic axis that level l (grid d) cannot coarsen: P1per needs an even length of at least 4
std::string periodic_level_error(int l, int dim, const int64_t d[3], uint32_t mask, uint32_t periodic) {
  for (int a = 0; a < dim; ++a)
    if (((mask & periodic) >> a) & 1u)
      if (d[a] < 4 || (d[a] & 1))
        return "level " + std::to_string(l) + ": `periodic_axes` = " + std::to_string(periodic) + " makes axis " +
               std::string(1, "xyz"[a]) + " periodic, and it has " + std::to_string(d[a]) +
               " points on this level; a coarsened periodic axis needs an even length of at least 4 (the grid is " +
               std::to_string(d[0]) + " x " + std::to_string(d[1]) + " x " + std::to_string(d[2]) + ")";
  return "";
}

// What a constructor asks of the hierarchy beyond A, b, n_levels and the options.
struct HierarchySpec {
  // amg_hip_create_custom: the transfer operators of every level, else the built-in ones
  const int32_t* const* Pc = nullptr;
  const int32_t* const* Pr = nullptr;
  const double* const* Pv = nullptr;
  const int32_t* const* Rc = nullptr;
  const int32_t* const* Rr = nullptr;
  const double* const* Rv = nullptr;
  // amg_hip_create_rs (theta >= 0): strength-based C/F coarsening, n_levels is an upper bound
  double rs_theta = -1.0;
  int64_t rs_min_coarse = 0;
  // the tensor constructors: the grid of level 0 (dim 0: the flat index is coarsened), the
  // semi-coarsening rule (null: every axis), the periodic axes
  int dim = 0;
  const int64_t* dims = nullptr;
  const SemiRule* semi = nullptr;
  uint32_t periodic = 0;
  bool periodic_ctor = false;  // amg_hip_create_tensor_periodic or _periodic_dev: takes `cyclic_lines`
};

// ---- the pieces the constructors share; each front end calls them in its own order ----
// the `out` pointer of a constructor and its options, the caller's or the defaults
amg_hip_status out_and_options(const amg_hip_options* opts, amg_hip_solver** out, amg_hip_options* o) {
  if (!out) return fail(AMG_HIP_EINVAL, "out handle pointer is null");
  *out = nullptr;
  if (opts) *o = *opts;
  else amg_hip_default_options(o);
  return AMG_HIP_OK;
}
// full coarsening: every axis of the grid d can be halved
bool full_level_ok(int dim, const int64_t d[3]) { return d[0] >= 2 && d[1] >= 2 && (dim != 3 || d[2] >= 2); }
// "" or why level l (grid d) cannot coarsen the axes `mask`: a mask of the semi-coarsening rule, else all axes
std::string level_mask_error(int l, int dim, const int64_t d[3], int64_t mask, bool semi) {
  if (semi) return semi_mask_error(l, dim, d, mask);
  return full_level_ok(dim, d) ? "" : tensor_level_error(l, d);
}
// The levels of a hierarchy whose masks are known up front (masks null: full coarsening), walked
// before any device call: "" or what the first level that cannot coarsen says, in the level loops'
// words.  `who` goes in front of what only a front end can name: a mask, a periodic axis.
// one_axis (amg_hip_create_tensor_opdep): every mask names exactly one axis
std::string level_walk_error(const std::string& who, int dim, const int64_t* dims, int32_t n_levels,
                             const int32_t* masks, uint32_t periodic, bool one_axis = false) {
  int64_t d[3] = {dims[0], dims[1], dims[2]};
  for (int l = 0; l + 1 < n_levels; ++l) {
    const uint32_t mask = masks ? (uint32_t)masks[l] : tensor_full_mask(dim);
    std::string e = level_mask_error(l, dim, d, masks ? (int64_t)masks[l] : (int64_t)mask, masks != nullptr);
    if (e.empty() && one_axis && masks && (mask & (mask - 1u)))
      e = "level " + std::to_string(l) + ": axis mask " + std::to_string(masks[l]) +
          " names several axes; a level of this hierarchy coarsens exactly one (1, 2 or 4)";
    if (!e.empty()) return masks ? who + e : e;
    e = periodic_level_error(l, dim, d, mask, periodic);
    if (!e.empty()) return who + e;
    int64_t c[3];
    tensor_coarse_dims(dim, d, mask, c);
    for (int a = 0; a < 3; ++a) d[a] = c[a];
  }
  return "";
}
// The options of a constructor with the grid dimension tensor_dim (0: none) and n_levels levels, in
// the one order every constructor reports them.
amg_hip_status smoother_options_error(const amg_hip_options& o, int tensor_dim, int32_t n_levels,
                                      uint32_t periodic = 0, bool periodic_ctor = false) {
  if (o.smoother < 0 || o.smoother > AMG_HIP_SM_LINE_ALT) return fail(AMG_HIP_EINVAL, "unknown smoother kind");
  {
    const std::string e = sides_error(o, tensor_dim, periodic, periodic_ctor);
    if (!e.empty()) return fail(AMG_HIP_EINVAL, e);
    if (o.singular && n_levels < 2) return fail(AMG_HIP_EINVAL, SINGULAR_ONE_LEVEL);
  }
  const bool alt = o.smoother == AMG_HIP_SM_LINE_ALT;
  if (alt && !tensor_dim) return fail(AMG_HIP_EINVAL, ALT_NEEDS_GRID);
  if (o.smoother_iters < 0) return fail(AMG_HIP_EINVAL, "`smoother_iters` must be >= 0");
  if (o.smoother == AMG_HIP_SM_CHEBYSHEV) {
    const std::string e = cheb_options_error(o.cheb_degree, o.cheb_lower, o.cheb_upper);
    if (!e.empty()) return fail(AMG_HIP_EINVAL, e);
    if (o.window) return fail(AMG_HIP_EUNSUPPORTED, "the Chebyshev smoother is not available in a window solver");
  }
  if (o.smoother == AMG_HIP_SM_LINE_JACOBI || alt) {
    const std::string e = line_options_error(o.omega);
    if (!e.empty()) return fail(AMG_HIP_EINVAL, e);
    if (o.window) return fail(AMG_HIP_EUNSUPPORTED, "the line smoother is not available in a window solver");
  }
  if (o.layout < AMG_HIP_LAYOUT_AUTO || o.layout > AMG_HIP_LAYOUT_DICT)
    return fail(AMG_HIP_EINVAL, "unknown matrix layout");
  if (o.smoother == AMG_HIP_SM_SOR && (o.omega > 2 || o.omega < 0))
    return fail(AMG_HIP_EINVAL, "`omega` must be in [0, 2] but got omega=" + std::to_string(o.omega) +
                                    "\n");  // smoother.hpp:286-293
  return AMG_HIP_OK;
}
// binds the solver to the device and the stream its options name
amg_hip_status bind_device(amg_hip_solver* s) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(AMG_HIP_EHIP, "no HIP device available (this library has no CPU fallback)");
  if (s->opt.device >= 0) {
    if (s->opt.device >= ndev) return fail(AMG_HIP_EINVAL, "device ordinal out of range");
    s->device = s->opt.device;
  } else {
    HIP_TRY(hipGetDevice(&s->device));
  }
  HIP_TRY(hipSetDevice(s->device));
  if (s->opt.stream) {
    s->stream = (hipStream_t)s->opt.stream;
    s->own_stream = false;
  } else {
    HIP_TRY(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
  }
  return AMG_HIP_OK;
}
// The axes level L (not the last) of a tensor hierarchy coarsens: all of them, the rule's explicit
// mask, or the automatic rule's from the three axis strengths that strengths(w) yields (the host
// loop from its CSR copy, the device loop from K-AxisStrength).  *last: the rule ends the hierarchy here.
template <class Strengths>
amg_hip_status level_axis_mask(const Level& L, int l, int dim, const SemiRule* semi, Strengths&& strengths,
                               uint32_t* mask, bool* last) {
  *last = false;
  *mask = tensor_full_mask(dim);
  if (semi && semi->masks) {
    *mask = (uint32_t)semi->masks[l];
  } else if (semi) {  // the hierarchy ends at a small level or when no axis is eligible
    *last = L.n <= semi->min_coarse;
    if (!*last) {
      double w[3];
      AMG_TRY(strengths(w));
      *mask = semi->opdep ? tensor_opdep_auto_mask(dim, L.dims, w, L.tper) : tensor_auto_mask(dim, L.dims, w, semi->theta);
      *last = *mask == 0;
    }
    if (*last) *mask = 0;
  }
  return AMG_HIP_OK;
}
// u, f, r (zeroed) and tmp of a level, and the Chebyshev smoother's update vector
amg_hip_status alloc_level_vectors(Level& L, bool cheb) {
  HIP_TRY(L.u.alloc(sizeof(double) * L.n));
  HIP_TRY(L.f.alloc(sizeof(double) * L.n));
  HIP_TRY(L.r.alloc(sizeof(double) * L.n));
  HIP_TRY(L.tmp.alloc(sizeof(double) * L.n));
  HIP_TRY(hipMemset(L.u.p, 0, sizeof(double) * L.n));
  HIP_TRY(hipMemset(L.f.p, 0, sizeof(double) * L.n));
  HIP_TRY(hipMemset(L.r.p, 0, sizeof(double) * L.n));
  if (cheb) {
    HIP_TRY(L.cheb_d.alloc(sizeof(double) * L.n));
    HIP_TRY(hipMemset(L.cheb_d.p, 0, sizeof(double) * L.n));
  }
  return AMG_HIP_OK;
}
// K-GS-scan on the dictionary matrix A: the chunk length and the ring of new values, or false
// when the chunks would be too short or the ring would not fit the LDS
bool gs_scan_params(const DevMat& A, int* C_out, int* ring_out) {
  int ring = 128;
  int C = (int)std::min<int64_t>(A.scan_gap, gs_scan_long_chunks_ok(A.dict_ref()) ? gs_scan_max_chunk() : 1024);
  if (C > 1024 && A.scan_far + C + 1 > 16384) C = 1024;  // the ring of new values must fit the LDS
  while (ring < A.scan_far + C + 1 && ring <= 16384) ring *= 2;
  if (A.scan_gap < GS_SCAN_MIN_GAP || ring > 16384) return false;
  *C_out = C;
  *ring_out = ring;
  return true;
}
// The closing steps of a set-up on a device: the coarsest factor (multigrid.hpp:240-243; no window
// solver has one), scratch, the K-Patch flags, the bytes model.  coarse_done() laps the caller's timer.
template <class Lap>
amg_hip_status finish_device_solver(amg_hip_solver* s, Lap&& coarse_done) {
  if (!s->opt.window) {
    const int want = s->opt.fast_coarse_solve ? 1 : (s->opt.exact_coarse_solve ? -1 : 0);
    AMG_TRY(upload_coarse(s->lv.back().A_csc, want, &s->coarse, s->opt.singular != 0));
  }
  coarse_done();
  HIP_TRY(s->scratch.alloc(sizeof(double) * 1100));
  AMG_TRY(set_patch_coarse_flags(s));
  compute_bytes(s);
  HIP_TRY(hipDeviceSynchronize());
  return AMG_HIP_OK;
}

amg_hip_status build_solver(int64_t n, const int32_t* colptr, const int32_t* rowind, const double* val,
                            const double* b, int32_t n_levels, const amg_hip_options* opts, amg_hip_solver** out,
                            const HierarchySpec& h = HierarchySpec()) {
  std::unique_ptr<amg_hip_solver> s(new amg_hip_solver);
  AMG_TRY(out_and_options(opts, out, &s->opt));
  if (!colptr || !rowind || !val || !b) return fail(AMG_HIP_EINVAL, "null input array");
  const bool rs = h.rs_theta >= 0.0;
  if (n <= 0) return fail(AMG_HIP_EINVAL, "`A` must have at least one degree of freedom");
  if (n_levels < 1) return fail(AMG_HIP_EINVAL, "`n_levels` must be at least 1");
  AMG_TRY(smoother_options_error(s->opt, h.dim, n_levels, h.periodic, h.periodic_ctor));
  const bool alt = s->opt.smoother == AMG_HIP_SM_LINE_ALT;
  const bool cheb = s->opt.smoother == AMG_HIP_SM_CHEBYSHEV;
  const bool line = s->opt.smoother == AMG_HIP_SM_LINE_JACOBI;
  const bool dev = !s->opt.host_only;
  if (dev) AMG_TRY(bind_device(s.get()));

  // AMG_HIP_TIMING=1: wall time of the setup phases on stderr
  struct PhaseTimer {
    bool on = std::getenv("AMG_HIP_TIMING") != nullptr;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    std::vector<std::pair<const char*, double>> acc;
    void lap(const char* name) {
      if (!on) return;
      const auto t1 = std::chrono::steady_clock::now();
      const double dt = std::chrono::duration<double>(t1 - t0).count();
      t0 = t1;
      for (auto& a : acc)
        if (a.first == name) { a.second += dt; return; }
      acc.emplace_back(name, dt);
    }
    ~PhaseTimer() {
      if (!on) return;
      std::fprintf(stderr, "amg_hip setup:");
      for (auto& a : acc) std::fprintf(stderr, " %s %.2fs", a.first, a.second);
      std::fprintf(stderr, "\n");
    }
  } timer;
  static const char *T_IN = "input+transpose", *T_ENC = "encode+upload", *T_SM = "smoother-setup",
                    *T_TR = "transfers", *T_RAP = "galerkin", *T_CSC = "csc-copy", *T_BAND = "band";
  const int nt = host_threads();
  s->lv.resize(n_levels);
  {
    Level& L0 = s->lv[0];
    L0.n = n;
    L0.A_csc = from_raw(n, n, colptr, rowind, val);
    std::string v = validate(L0.A_csc, "A");
    if (!v.empty()) return fail(AMG_HIP_EINVAL, v);
    if (h.dim) {
      L0.tdim = h.dim;
      for (int a = 0; a < 3; ++a) L0.dims[a] = h.dims[a];
    }
  }
  // ---- hierarchy (multigrid.hpp:211-237) ----
  Sparse A_r = transpose(s->lv[0].A_csc);  // CSR(A_0)
  DevCsr galerkin_A;             // CSR(A_l) on the device while the Galerkin chain runs there
  bool galerkin_on_dev = false;
  timer.lap(T_IN);
  for (int l = 0; l < n_levels; ++l) {
    Level& L = s->lv[l];
    if (h.dim) L.tsides = (uint32_t)s->opt.natural_sides;
    if (h.dim) L.tper = h.periodic;
    if (h.dim && l + 1 < n_levels) {  // the axes this level coarsens
      bool last = false;
      AMG_TRY(level_axis_mask(L, l, h.dim, h.semi, [&](double w[3]) {
        tensor_axis_strength(A_r, h.dim, L.dims, w);
        return AMG_HIP_OK;
      }, &L.tmask, &last));
      if (last) {
        n_levels = l + 1;
        s->lv.resize((size_t)n_levels);
      }
    }
    L.symmetric = same_arrays(A_r, L.A_csc);
    L.nnz_struct = L.A_csc.nnz();
    if (cheb) {  // bound of D^-1 A from the rows of A_l (CSR(A_l) = A_r)
      int64_t zr = -1;
      const double G = gershgorin_host(A_r, &zr);
      if (zr >= 0) return fail(AMG_HIP_EINVAL, cheb_zero_diag(l, zr));
      L.cheb_lo = s->opt.cheb_lower * G;
      L.cheb_hi = s->opt.cheb_upper * G;
    }
    if (line && !dev) {  // host_only: the stride and the pivot check on the host
      if (L.n >= ((int64_t)1 << 31)) return fail(AMG_HIP_EUNSUPPORTED, "line smoother: levels of 2^31 rows or more");
      L.line.n = L.n;
      L.line.s = line_stride_host(L.n, A_r.ptr.data(), A_r.idx.data(), A_r.val.data());
      const int64_t bad = line_setup_host(L.n, L.line.s, A_r.ptr.data(), A_r.idx.data(), A_r.val.data());
      if (bad >= 0) return fail(AMG_HIP_EINVAL, line_bad_pivot(l, bad));
    }
    if (line && dev) {  // the same device setup as amg_hip_create_poisson, from a CSR copy of the rows
      if (L.n >= ((int64_t)1 << 31)) return fail(AMG_HIP_EUNSUPPORTED, "line smoother: levels of 2^31 rows or more");
      DevCsr rows;
      HIP_TRY(upload_csr(A_r, &rows));
      const amg_hip_status lr = line_setup_dev(l, L.n, rows.rowptr(), rows.col(), rows.v(), 0, &L.line);
      if (lr != AMG_HIP_OK) return lr;
    }
    if (alt) {  // directions of the level's grid; pivot check on the host (host_only) or the device set-up
      if (L.n >= ((int64_t)1 << 31)) return fail(AMG_HIP_EUNSUPPORTED, "line smoother: levels of 2^31 rows or more");
      L.alt.set_grid(L.n, L.dims, s->opt.cyclic_lines ? h.periodic : 0u);
      if (!dev) {
        const amg_hip_status ar = alt_setup_host(l, A_r.ptr.data(), A_r.idx.data(), A_r.val.data(), &L.alt);
        if (ar != AMG_HIP_OK) return ar;
      } else {
        DevCsr rows;
        HIP_TRY(upload_csr(A_r, &rows));
        const amg_hip_status ar = alt_setup_dev(l, rows.rowptr(), rows.col(), rows.v(), &L.alt);
        if (ar != AMG_HIP_OK) return ar;
      }
    }
    if (dev) {
    const bool prune = !s->opt.keep_structural_zeros;
    // Symmetric levels headed for the dictionary layout are encoded ON THE DEVICE from CSR(A_l)
    // (K-Setup: the encoder kernels check every row against a table proposed from a sample of
    // rows); the arrays are there anyway for the Galerkin chain.  Everything else takes the
    // host encoder.
    bool encoded = false;
    if (L.symmetric && (s->opt.layout == AMG_HIP_LAYOUT_AUTO || s->opt.layout == AMG_HIP_LAYOUT_DICT) &&
        L.n >= (1 << 16) && A_r.nnz() < ((int64_t)1 << 31) - 1) {
      if (!galerkin_on_dev) {
        HIP_TRY(upload_csr(A_r, &galerkin_A));
        galerkin_on_dev = true;
      }
      DevMem stats;
      HIP_TRY(stats.alloc(sizeof(int32_t) * 2));
      HIP_TRY(hipMemset(stats.p, 0, sizeof(int32_t) * 2));
      HIP_TRY(L.diag.alloc(sizeof(double) * L.n));
      HIP_TRY(launch_csr_inspect(L.n, galerkin_A.rowptr(), galerkin_A.col(), galerkin_A.v(), prune,
                                 stats.as<int32_t>(), L.diag.as<double>(), nullptr));
      int32_t st2[2];
      HIP_TRY(hipMemcpy(st2, stats.p, sizeof(st2), hipMemcpyDeviceToHost));
      if (st2[1] == 0) HIP_TRY(device_dict_encode(galerkin_A, prune, st2[0], &L.A_rows, &encoded));
      if (!encoded || s->opt.smoother != AMG_HIP_SM_JACOBI) L.diag.release();
    }
    if (!encoded) {
      HIP_TRY(upload_mat_pruned(A_r, s->opt.layout, prune, &L.A_rows));
      if (!L.symmetric && s->opt.smoother >= AMG_HIP_SM_JACOBI && !cheb && !line && !alt)  // Chebyshev, line: rows of A
        HIP_TRY(upload_mat_pruned(L.A_csc, s->opt.layout, prune, &L.A_cols_own));
    }
    if (s->opt.smoother == AMG_HIP_SM_JACOBI && !L.diag.p) {  // diagonal of the column-as-row walk
      std::vector<double> dg(L.n, 0.0);
      for (int64_t c = 0; c < L.n; ++c)
        for (int32_t p = L.A_csc.ptr[c]; p < L.A_csc.ptr[c + 1]; ++p)
          if (L.A_csc.idx[p] == c) dg[c] = L.A_csc.val[p];
      HIP_TRY(upload(L.diag, dg.data(), dg.size()));
    }
    AMG_TRY(alloc_level_vectors(L, cheb));
    timer.lap(T_ENC);
    // smoother-specific structures
    // Lexicographic sweeps at size: the line-scan form, unless opt.exact_gs or a small
    // problem (the exact dependency-scheduled kernel is bit-exact and fast enough there)
    if (s->opt.smoother <= AMG_HIP_SM_SOR && !s->opt.exact_gs && s->lv[0].n > GS_SCAN_MIN_ROWS &&
        L.symmetric && L.A_rows.dict && L.A_rows.dict_shift == 0)
      (void)gs_scan_params(L.A_rows, &L.scan_C, &L.scan_ring);
    if (L.scan_C > 0) {
      // no schedule needed
    } else if (s->opt.smoother == AMG_HIP_SM_SPGS) {
      LexSchedule F, B;
      std::string e = build_lex_schedule(L.A_csc, false, 64, &F);
      if (e.empty()) e = build_lex_schedule(L.A_csc, true, 64, &B);
      if (!e.empty()) return fail(AMG_HIP_EUNSUPPORTED, e);
      L.lex_fwd.reset(new LexOnDev);
      L.lex_bwd.reset(new LexOnDev);
      HIP_TRY(upload_lex(F, L.lex_fwd.get()));
      HIP_TRY(upload_lex(B, L.lex_bwd.get()));
    } else if (s->opt.smoother == AMG_HIP_SM_REF_JACOBI || s->opt.smoother == AMG_HIP_SM_SOR) {
      LexSchedule F;  // these two address A by ROW (A.coeff(i,j), smoother.hpp:251,351)
      std::string e = build_lex_schedule(A_r, false, 64, &F);
      if (!e.empty()) return fail(AMG_HIP_EUNSUPPORTED, e);
      L.lex_fwd.reset(new LexOnDev);
      HIP_TRY(upload_lex(F, L.lex_fwd.get()));
    } else if (s->opt.smoother == AMG_HIP_SM_MULTICOLOR_GS) {
      greedy_coloring(L.A_csc, &L.color, &L.n_colors);
      // K-Patch form of the passes (patch_rb_kernel): the colour of a row is a function of the
      // parities of its grid line and column
      L.mc_ctab = -1;
      if (L.n_colors <= 4 && L.A_rows.patch && L.symmetric && (L.A_rows.patch_m % 2) == 0 &&
          L.A_rows.patch_m >= 8 && L.n >= 2 * L.A_rows.patch_m) {
        const int64_t m = L.A_rows.patch_m;
        auto cls = [m](int64_t c) -> int {
          return c == 0 ? 0 : (c == 1 ? 1 : (c == m - 2 ? 2 : (c == m - 1 ? 3 : 4 + (int)(c & 1))));
        };
        int32_t tab[12];
        const int64_t sample[6] = {0, 1, m - 2, m - 1, 2, 3};
        for (int p = 0; p < 2; ++p)
          for (int q = 0; q < 6; ++q) tab[p * 6 + q] = L.color[(size_t)(p * m + sample[q])];
        bool ok = true;
        for (int64_t i0 = 0, line = 0; i0 < L.n && ok; i0 += m, ++line) {
          const int32_t* t = tab + 6 * (line & 1);
          const int32_t* c = L.color.data() + i0;
          const int64_t len = std::min<int64_t>(m, L.n - i0);
          for (int64_t j = 0; j < len; ++j) ok &= c[j] == t[(j < 2 || j >= m - 2) ? cls(j) : 4 + (j & 1)];
        }
        if (ok) {
          L.mc_ctab = 0;
          for (int q = 0; q < 12; ++q) L.mc_ctab |= tab[q] << (2 * q);
          if (s->opt.keep_residual && L.n >= s->patch_min_rows) HIP_TRY(L.mc_aux.alloc(sizeof(double) * L.n));
        }
      }
      if (L.n_colors <= 15 && !(L.mc_ctab >= 0 && L.n >= s->patch_min_rows)) {  // K-Strip's colour bytes
        std::vector<uint8_t> c8((size_t)L.n);
        for (int64_t i = 0; i < L.n; ++i) c8[(size_t)i] = (uint8_t)L.color[(size_t)i];
        HIP_TRY(upload(L.mc_color8, c8.data(), c8.size()));
      }
      ColorPerm CP;
      build_color_perm(L.A_csc, L.color, L.n_colors, &CP);  // column-as-row walk, like SpGS
      if (CP.rows.n_outer >= ((int64_t)1 << 31) - 512)
        return fail(AMG_HIP_EUNSUPPORTED, "multicolour smoother: level too large for int32 rows");
      DictMat T;
      L.mc_dict = (s->opt.layout == AMG_HIP_LAYOUT_AUTO || s->opt.layout == AMG_HIP_LAYOUT_DICT) &&
                  to_dict(CP.rows, 0, &T, CP.rowid.data());
      if (L.mc_dict) {
        L.mc_words = T.words;
        L.mc_wmax = T.max_width;
        L.mc_ntab = (int)T.doff.size();
        HIP_TRY(upload(L.mc_codes, T.codes.data(), T.codes.size()));
        HIP_TRY(upload(L.mc_doff, T.doff.data(), T.doff.size()));
        HIP_TRY(upload(L.mc_dval, T.dval.data(), T.dval.size()));
      } else {
        HIP_TRY(upload_mat(CP.rows, AMG_HIP_LAYOUT_SELL, &L.mc_mat, 0, false));
      }
      HIP_TRY(upload(L.mc_rowid, CP.rowid.data(), CP.rowid.size()));
      L.mc_start = CP.start;
      if (L.mc_dict && L.n <= mc_one_launch_max_rows()) {
        std::vector<int32_t> st32(CP.start.begin(), CP.start.end());
        HIP_TRY(upload(L.mc_start_dev, st32.data(), st32.size()));
      }
    }
    }  // dev
    if (!dev && s->opt.smoother == AMG_HIP_SM_MULTICOLOR_GS)
      greedy_coloring(L.A_csc, &L.color, &L.n_colors);
    timer.lap(T_SM);
    if (l + 1 == n_levels) break;
    // ---- transfer operators for level l -> l+1 ----
    const int64_t n_h = L.n;
    int64_t n_H = coarse_dofs(n_h);  // multigrid.hpp:214
    if (rs) {
      // host_setup.hpp: ruge_stueben_P.  The hierarchy ends where a level is small enough for
      // the direct solve or no longer coarsens.
      bool last = n_h <= h.rs_min_coarse;
      if (!last) {
        L.P_csc = ruge_stueben_P(A_r, h.rs_theta);
        n_H = L.P_csc.n_outer;
        last = n_H < 1 || n_H >= n_h;
      }
      if (last) {
        L.P_csc = Sparse();
        n_levels = l + 1;
        s->lv.resize((size_t)n_levels);
        break;
      }
      L.R_csc = transpose(L.P_csc);
      L.linear = false;
    } else if (h.dim) {
      // every coarsened axis m -> floor(m / 2), possible while it has 2 points
      const std::string e = level_mask_error(l, h.dim, L.dims, L.tmask, h.semi != nullptr);
      if (!e.empty()) return fail(AMG_HIP_EINVAL, e);
      Level& C = s->lv[l + 1];
      C.tdim = h.dim;
      tensor_coarse_dims(h.dim, L.dims, L.tmask, C.dims);
      n_H = C.dims[0] * C.dims[1] * C.dims[2];
      L.tensor = true;
      L.n_coarse = n_H;
      // the matrix-free kernels index lanes with 32 bits (kernels.hip: tensor_grid)
      L.tensor_stencil = s->opt.stencil_transfers && L.n < ((int64_t)1 << 31) - 4;
      if (h.semi && h.semi->opdep) {  // one axis, the weights of this level's rows; kind 3 or 0
        L.axis_stencil = L.tensor_stencil && g_axis_stencil;
        L.tensor_stencil = false;
        for (L.axis = 0; !((L.tmask >> L.axis) & 1u); ++L.axis) {}
        const std::string we = axis_opdep_P(A_r, h.dim, L.dims, L.axis, &L.P_csc, &L.axis_W, L.axis_periodic());
        if (!we.empty()) return fail(AMG_HIP_EINVAL, std::string(h.semi->opdep_who) + "level " + std::to_string(l) + ": " + we);
        L.R_csc = transpose(L.P_csc);
        if (dev && L.axis_stencil) HIP_TRY(upload(L.axis_W_dev, L.axis_W.data(), L.axis_W.size()));
      } else if (!L.tensor_stencil) {
        L.P_csc = tensor_P(h.dim, L.dims, L.tmask, L.tsides, L.tper);
        L.R_csc = transpose(L.P_csc);
      }
    } else if (n_H < 1) {
      return fail(AMG_HIP_EINVAL, "level " + std::to_string(l + 1) +
                                      " would have no degrees of freedom; reduce `n_levels`");
    } else if (h.Pc) {
      // The arrays carry no coarse size.  The reference's rule is the default; operators of another
      // coarsening (full coarsening of a grid, aggregation) say theirs through R_l, whose rows are
      // the coarse dofs: largest row index + 1.
      if (h.Rc[l] && h.Rr[l]) {
        int64_t rows = 0;
        for (int32_t q = 0, e = h.Rc[l][n_h]; q < e; ++q) rows = std::max<int64_t>(rows, (int64_t)h.Rr[l][q] + 1);
        if (rows >= 1 && rows != n_H) n_H = rows;
      }
      L.P_csc = from_raw(n_H, n_h, h.Pc[l], h.Pr[l], h.Pv[l]);
      L.R_csc = from_raw(n_h, n_H, h.Rc[l], h.Rr[l], h.Rv[l]);
      std::string v = validate(L.P_csc, "P");
      if (v.empty()) v = validate(L.R_csc, "R");
      if (!v.empty()) return fail(AMG_HIP_EINVAL, v);
      L.linear = is_linear_P(L.P_csc, n_h, n_H) && same_arrays(transpose(L.P_csc), L.R_csc);
    } else {
      L.lazy_linear = true;
      L.n_coarse = n_H;
      L.linear = true;
    }
    // the matrix-free kernels need no device copy of the linear operators, and the
    // device Galerkin product no host copy
    const bool dev_galerkin = dev && L.linear && !s->opt.host_galerkin;
    const bool dev_rows = dev && !(L.linear && s->opt.stencil_transfers) && !L.tensor_stencil && !L.axis_stencil;
    Sparse P_r, R_r;
    if (dev_rows || !dev_galerkin) {
      P_r = transpose(L.P());  // CSR(P)
      R_r = transpose(L.R());  // CSR(R)
    }
    if (dev_rows) {
      HIP_TRY(upload_csr(P_r, &L.P_rows));
      HIP_TRY(upload_csr(R_r, &L.R_rows));
    }
    timer.lap(T_TR);
    // Galerkin (multigrid.hpp:219-223), row-major, Eigen's summation order: on the device
    // for the linear interpolation pair (K-Galerkin), else on the host (same bits)
    Sparse AH_r;
    bool done = false;
    if (dev_galerkin) {
      if (!galerkin_on_dev) HIP_TRY(upload_csr(A_r, &galerkin_A));
      DevCsr next;
      HIP_TRY(device_galerkin(galerkin_A, n_H, &next, &AH_r));
      galerkin_A = std::move(next);
      galerkin_on_dev = true;
      done = true;
    } else if (dev && dev_rows && !s->opt.host_galerkin && !L.tensor) {
      // custom interpolator: general K-way-merge product on the device (CSR(P), CSR(R) were
      // uploaded for the transfer kernels anyway)
      if (!galerkin_on_dev) HIP_TRY(upload_csr(A_r, &galerkin_A));
      DevCsr next;
      HIP_TRY(device_galerkin_generic(galerkin_A, L.P_rows, L.R_rows, &next, &AH_r, &done));
      if (done) {
        galerkin_A = std::move(next);
        galerkin_on_dev = true;
      }
    }
    if (!done) {
      AH_r = galerkin_csr(R_r, A_r, P_r, nt);
      galerkin_on_dev = false;
    }
    if (L.tensor_stencil) {  // rebuilt when a getter or the block cycle asks (Level::P)
      L.P_csc = Sparse();
      L.R_csc = Sparse();
    }
    timer.lap(T_RAP);
    Level& C = s->lv[l + 1];
    C.n = n_H;
    C.A_csc = transpose(AH_r);
    timer.lap(T_CSC);
    A_r.ptr.swap(AH_r.ptr);
    A_r.idx.swap(AH_r.idx);
    A_r.val.swap(AH_r.val);
    A_r.n_outer = A_r.n_inner = n_H;
  }
  // the automatic semi-coarsening rule may have stopped at level 0
  if (s->opt.singular && n_levels < 2) return fail(AMG_HIP_EINVAL, SINGULAR_ONE_LEVEL);
  if (!dev) {
    compute_bytes(s.get());
    *out = s.release();
    return AMG_HIP_OK;
  }
  // rhs / initial state (multigrid.hpp:196-204)
  HIP_TRY(hipMemcpy(s->lv[0].f.p, b, sizeof(double) * n, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(s->lv[0].r.p, b, sizeof(double) * n, hipMemcpyHostToDevice));  // b - A*0
  AMG_TRY(finish_device_solver(s.get(), [&] { timer.lap(T_BAND); }));
  *out = s.release();
  return AMG_HIP_OK;
}

// ---- setup on the device end to end (amg_hip_create_poisson) -------------------
// Dictionary encoding of CSR(A) that sits on the device (K-Setup: dict_encode_kernel,
// dict_type_kernel).  The pair table and the word table are PROPOSED by the host from a
// sample of rows (first and last 64 K) and VERIFIED by the kernels on every row; rows that
// do not encode are reported back, their pairs / words are added, and the pass is repeated.
// Returns false (D untouched in the sense of dict = false) when the matrix does not qualify.
struct HostRows {  // rows [r0, r1) of a device CSR matrix
  int64_t r0 = 0;
  std::vector<int32_t> ptr, col;
  std::vector<double> val;
};
hipError_t fetch_rows(const DevCsr& A, int64_t r0, int64_t r1, HostRows* R) {
  R->r0 = r0;
  R->ptr.resize((size_t)(r1 - r0 + 1));
  hipError_t e = hipMemcpy(R->ptr.data(), A.rowptr() + r0, sizeof(int32_t) * R->ptr.size(), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return e;
  const int64_t p0 = R->ptr.front(), p1 = R->ptr.back();
  R->col.resize((size_t)(p1 - p0));
  R->val.resize((size_t)(p1 - p0));
  if (p1 > p0) {
    if ((e = hipMemcpy(R->col.data(), A.col() + p0, sizeof(int32_t) * (p1 - p0), hipMemcpyDeviceToHost)) != hipSuccess) return e;
    if ((e = hipMemcpy(R->val.data(), A.v() + p0, sizeof(double) * (p1 - p0), hipMemcpyDeviceToHost)) != hipSuccess) return e;
  }
  return hipSuccess;
}
hipError_t device_dict_encode(const DevCsr& A, bool prune, int maxlen, DevMat* D, bool* ok) {
  *ok = false;
  const int64_t n = A.n_rows;
  if (maxlen > 16 || n >= ((int64_t)1 << 28) || n < 1) return hipSuccess;
  hipError_t e;
  DictMat T;
  T.n = n;
  T.max_width = maxlen;
  T.words = maxlen > 8 ? 2 : 1;
  const int nw = T.words;
  std::map<std::pair<int32_t, uint64_t>, int> pairs;
  auto add_pairs = [&](const HostRows& R) {
    for (size_t r = 0; r + 1 < R.ptr.size(); ++r) {
      if (T.doff.size() > 255) return;  // does not qualify: no need to number the rest of the sample
      for (int32_t p = R.ptr[r] - R.ptr[0]; p < R.ptr[r + 1] - R.ptr[0]; ++p) {
        if (prune && R.val[p] == 0.0) continue;
        uint64_t bits;
        std::memcpy(&bits, &R.val[p], 8);
        const auto key = std::make_pair((int32_t)((int64_t)R.col[p] - (R.r0 + (int64_t)r)), bits);
        if (pairs.emplace(key, (int)T.doff.size()).second) {
          T.doff.push_back(key.first);
          T.dval.push_back(R.val[p]);
        }
      }
    }
  };
  const int64_t S = std::min<int64_t>(n, 65536);
  HostRows R;
  if ((e = fetch_rows(A, 0, S, &R)) != hipSuccess) return e;
  add_pairs(R);
  if (n > S) {
    if ((e = fetch_rows(A, n - S, n, &R)) != hipSuccess) return e;
    add_pairs(R);
  }
  DevMem dfail, dcodes, doff, dval;
  int32_t fail[64];
  if ((e = dfail.alloc(sizeof(fail))) != hipSuccess) return e;
  if ((e = dcodes.alloc(sizeof(uint64_t) * (size_t)n * nw)) != hipSuccess) return e;
  for (int round = 0;; ++round) {
    if (T.doff.size() > 255 || round > 64) return hipSuccess;  // does not qualify
    if ((e = upload(doff, T.doff.data(), T.doff.size())) != hipSuccess) return e;
    if ((e = upload(dval, T.dval.data(), T.dval.size())) != hipSuccess) return e;
    if ((e = hipMemset(dfail.p, 0, sizeof(fail))) != hipSuccess) return e;
    if ((e = launch_dict_encode(n, A.rowptr(), A.col(), A.v(), prune, doff.as<int32_t>(),
                                dval.as<double>(), (int)T.doff.size(), nw, dcodes.as<uint64_t>(),
                                dfail.as<int32_t>(), nullptr)) != hipSuccess)
      return e;
    if ((e = hipMemcpy(fail, dfail.p, sizeof(fail), hipMemcpyDeviceToHost)) != hipSuccess) return e;
    if (fail[0] == 0) break;
    const size_t before = T.doff.size();
    for (int k = 0; k < std::min(fail[0], 62); ++k) {
      if ((e = fetch_rows(A, fail[1 + k], (int64_t)fail[1 + k] + 1, &R)) != hipSuccess) return e;
      add_pairs(R);
    }
    if (T.doff.size() == before) return hipSuccess;  // a row longer than the code words hold
  }
  // second level: row types
  T.rwords.assign((size_t)256 * nw, ~(uint64_t)0);
  std::map<std::pair<uint64_t, uint64_t>, int> types;
  auto add_words = [&](const std::vector<uint64_t>& cw) {
    for (size_t r = 0; r * nw < cw.size(); ++r) {
      const std::pair<uint64_t, uint64_t> key(cw[r * nw], nw == 2 ? cw[r * 2 + 1] : ~(uint64_t)0);
      if (key.first == ~(uint64_t)0 && key.second == ~(uint64_t)0) continue;  // empty row: type 255
      if (types.size() < 256 && types.emplace(key, (int)types.size()).second && types.size() <= 255) {
        const int ty = (int)types.size() - 1;
        T.rwords[(size_t)ty * nw] = key.first;
        if (nw == 2) T.rwords[(size_t)ty * 2 + 1] = key.second;
      }
    }
  };
  auto fetch_codes = [&](int64_t r0, int64_t r1, std::vector<uint64_t>* cw) -> hipError_t {
    cw->resize((size_t)(r1 - r0) * nw);
    return hipMemcpy(cw->data(), dcodes.as<uint64_t>() + r0 * nw, sizeof(uint64_t) * cw->size(), hipMemcpyDeviceToHost);
  };
  bool typed = g_row_types != 0;
  DevMem drtype, drwords;
  if (typed) {
    std::vector<uint64_t> cw;
    if ((e = fetch_codes(0, S, &cw)) != hipSuccess) return e;
    add_words(cw);
    if (n > S) {
      if ((e = fetch_codes(n - S, n, &cw)) != hipSuccess) return e;
      add_words(cw);
    }
    if ((e = drtype.alloc((size_t)n)) != hipSuccess) return e;
    for (int round = 0; typed; ++round) {
      if (types.size() > 255 || round > 64) { typed = false; break; }
      if ((e = upload(drwords, T.rwords.data(), T.rwords.size())) != hipSuccess) return e;
      if ((e = hipMemset(dfail.p, 0, sizeof(fail))) != hipSuccess) return e;
      if ((e = launch_dict_types(n, dcodes.as<uint64_t>(), nw, drwords.as<uint64_t>(), (int)types.size(),
                                 drtype.as<uint8_t>(), dfail.as<int32_t>(), nullptr)) != hipSuccess)
        return e;
      if ((e = hipMemcpy(fail, dfail.p, sizeof(fail), hipMemcpyDeviceToHost)) != hipSuccess) return e;
      if (fail[0] == 0) break;
      for (int k = 0; k < std::min(fail[0], 62); ++k) {
        if ((e = fetch_codes(fail[1 + k], (int64_t)fail[1 + k] + 1, &cw)) != hipSuccess) return e;
        add_words(cw);
      }
    }
  }
  D->n_rows = n;
  D->nnz = A.nnz;
  D->dict_typed = typed;
  if (typed) {
    D->drtype = std::move(drtype);
  } else {
    T.rwords.clear();
    D->dcodes = std::move(dcodes);
  }
  if ((e = finish_dict(T, n, 0, D)) != hipSuccess) return e;
  *ok = true;
  return hipSuccess;
}

// K-SellPack: what upload_mat(M, layout) uploads for the pruned CSR matrix M = A when it does not
// take the dictionary (SELL-64 panels or CSR by the same rule, the same index width and
// non-temporal bit, the same arrays bit for bit), made from the device arrays of A.  *ok = false:
// the panels need 2^31 slots or more; the caller takes the host upload.
hipError_t device_sell_pack(const DevCsr& A, int layout, bool prune, DevMat* D, bool* ok) {
  *ok = false;
  const int64_t n = A.n_rows;
  if (n < 1 || n >= ((int64_t)1 << 31) - 512) return hipSuccess;
  const int64_t np = (n + 63) / 64;
  hipError_t e;
  DevMem kept, pslots, stats, bsum, total, off32, optr;
  if ((e = kept.alloc(sizeof(int32_t) * (n + 1))) != hipSuccess) return e;
  if ((e = pslots.alloc(sizeof(int32_t) * (np + 1))) != hipSuccess) return e;
  if ((e = stats.alloc(sizeof(int32_t) * 3)) != hipSuccess) return e;
  if ((e = bsum.alloc(sizeof(int64_t) * ((n + 1023) / 1024 + 1))) != hipSuccess) return e;
  if ((e = total.alloc(sizeof(int64_t))) != hipSuccess) return e;
  if ((e = optr.alloc(sizeof(int32_t) * (n + 1))) != hipSuccess) return e;
  if ((e = off32.alloc(sizeof(int32_t) * (np + 1))) != hipSuccess) return e;
  if ((e = hipMemset(stats.p, 0, sizeof(int32_t) * 3)) != hipSuccess) return e;
  if ((e = launch_sell_count(n, A.rowptr(), A.col(), A.v(), prune, kept.as<int32_t>(), pslots.as<int32_t>(),
                             stats.as<int32_t>(), nullptr)) != hipSuccess)
    return e;
  int64_t nnz = 0, slots = 0;
  if ((e = launch_exclusive_scan(n, kept.as<int32_t>(), optr.as<int32_t>(), bsum.as<int64_t>(), total.as<int64_t>(),
                                 nullptr)) != hipSuccess)
    return e;
  if ((e = hipMemcpy(&nnz, total.p, sizeof(int64_t), hipMemcpyDeviceToHost)) != hipSuccess) return e;
  if ((e = launch_exclusive_scan(np, pslots.as<int32_t>(), off32.as<int32_t>(), bsum.as<int64_t>(),
                                 total.as<int64_t>(), nullptr)) != hipSuccess)
    return e;
  if ((e = hipMemcpy(&slots, total.p, sizeof(int64_t), hipMemcpyDeviceToHost)) != hipSuccess) return e;
  int32_t st[3];
  if ((e = hipMemcpy(st, stats.p, sizeof(st), hipMemcpyDeviceToHost)) != hipSuccess) return e;
  if (slots >= ((int64_t)1 << 31) - 1) return hipSuccess;  // the scan's offsets are 32-bit
  // upload_mat's rule: an explicit SELL or CSR request holds (a dictionary request that did not
  // qualify is a SELL request), AUTO takes SELL-64 unless padding exceeds 25 %
  bool sell = layout != AMG_HIP_LAYOUT_CSR;
  if (layout == AMG_HIP_LAYOUT_AUTO) sell = (double)slots <= 1.25 * (double)nnz + 4096.0;
  D->n_rows = n;
  D->nnz = nnz;
  D->dict = false;
  D->sell = sell;
  if (!sell) {
    DevCsr& C = D->csr;
    C.n_rows = n;
    C.n_cols = A.n_cols;
    C.nnz = nnz;
    C.max_block_nnz = st[2];
    C.max_row_nnz = st[0];
    if ((e = C.idx.alloc(sizeof(int32_t) * std::max<int64_t>(nnz, 1))) != hipSuccess) return e;
    if ((e = C.val.alloc(sizeof(double) * std::max<int64_t>(nnz, 1))) != hipSuccess) return e;
    if ((e = launch_csr_compact(n, A.rowptr(), A.col(), A.v(), prune, optr.as<int32_t>(), C.idx.as<int32_t>(),
                                C.val.as<double>(), nullptr)) != hipSuccess)
      return e;
    C.ptr = std::move(optr);
    *ok = true;
    return hipSuccess;
  }
  D->max_width = st[0];
  D->slots = slots;
  const bool fits = g_index16 != 0 && st[1] == 0;
  const double stream_bytes = (double)slots * (fits ? 10.0 : 12.0);
  D->idx16 = (fits ? 1 : 0) | ((g_nontemporal && stream_bytes > 192.0e6) ? 2 : 0);
  if ((e = D->soff.alloc(sizeof(int64_t) * (np + 1))) != hipSuccess) return e;
  if ((e = D->scol.alloc((size_t)slots * (fits ? sizeof(int16_t) : sizeof(int32_t)))) != hipSuccess) return e;
  if ((e = D->sval.alloc(sizeof(double) * (size_t)slots)) != hipSuccess) return e;
  if ((e = launch_sell_fill(n, A.rowptr(), A.col(), A.v(), prune, off32.as<int32_t>(), D->soff.as<int64_t>(), fits,
                            D->scol.p, D->sval.as<double>(), nullptr)) != hipSuccess)
    return e;
  if ((e = hipDeviceSynchronize()) != hipSuccess) return e;  // off32 is released on return
  *ok = true;
  return hipSuccess;
}

// K-Transpose: T = CSC(A) of the square device matrix A, equal to the host transpose(), structural
// zeros included.  *ok = false: a column has more entries than the kernel sorts.
hipError_t device_transpose(const DevCsr& A, DevCsr* T, bool* ok) {
  *ok = false;
  const int64_t n = A.n_rows, nnz = A.nnz;
  hipError_t e;
  DevMem cnt, bsum, total, ovf;
  if ((e = cnt.alloc(sizeof(int32_t) * (n + 1))) != hipSuccess) return e;
  if ((e = bsum.alloc(sizeof(int64_t) * ((n + 1023) / 1024 + 1))) != hipSuccess) return e;
  if ((e = total.alloc(sizeof(int64_t))) != hipSuccess) return e;
  if ((e = ovf.alloc(sizeof(int32_t))) != hipSuccess) return e;
  if ((e = hipMemset(cnt.p, 0, sizeof(int32_t) * (n + 1))) != hipSuccess) return e;
  if ((e = hipMemset(ovf.p, 0, sizeof(int32_t))) != hipSuccess) return e;
  if ((e = launch_transpose_count(nnz, A.col(), cnt.as<int32_t>(), nullptr)) != hipSuccess) return e;
  if ((e = T->ptr.alloc(sizeof(int32_t) * (n + 1))) != hipSuccess) return e;
  if ((e = launch_exclusive_scan(n, cnt.as<int32_t>(), T->ptr.as<int32_t>(), bsum.as<int64_t>(), total.as<int64_t>(),
                                 nullptr)) != hipSuccess)
    return e;
  if ((e = hipMemset(cnt.p, 0, sizeof(int32_t) * (n + 1))) != hipSuccess) return e;  // now the cursors
  if ((e = T->idx.alloc(sizeof(int32_t) * std::max<int64_t>(nnz, 1))) != hipSuccess) return e;
  if ((e = T->val.alloc(sizeof(double) * std::max<int64_t>(nnz, 1))) != hipSuccess) return e;
  if ((e = launch_transpose_fill(n, A.rowptr(), A.col(), A.v(), T->ptr.as<int32_t>(), cnt.as<int32_t>(),
                                 T->idx.as<int32_t>(), T->val.as<double>(), ovf.as<int32_t>(), nullptr)) != hipSuccess)
    return e;
  int32_t over = 0;
  if ((e = hipMemcpy(&over, ovf.p, sizeof(int32_t), hipMemcpyDeviceToHost)) != hipSuccess) return e;
  if (over) return hipSuccess;
  T->n_rows = T->n_cols = n;
  T->nnz = nnz;
  *ok = true;
  return hipSuccess;
}

void rhs_threads(int dim, int64_t n, double* b, int nt, int64_t d0 = 0, int64_t d1 = -1);  // below

// AMG_HIP_TIMING=1: wall time of the phases of a device set-up on stderr
struct SetupLap {
  bool on = std::getenv("AMG_HIP_TIMING") != nullptr;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  void operator()(const char* what) {
    if (!on) return;
    (void)hipDeviceSynchronize();
    const auto t1 = std::chrono::steady_clock::now();
    std::fprintf(stderr, "amg_hip device setup: %s %.3fs\n", what, std::chrono::duration<double>(t1 - t0).count());
    t0 = t1;
  }
};
// a solver with the options `o`, bound to its device and stream
amg_hip_status device_setup_begin(const amg_hip_options& o, std::unique_ptr<amg_hip_solver>* sp) {
  std::unique_ptr<amg_hip_solver> s(new amg_hip_solver);
  s->opt = o;
  AMG_TRY(bind_device(s.get()));
  *sp = std::move(s);
  return AMG_HIP_OK;
}

// The level loop of the device set-ups: from CSR(A_0) on the device (`cur`, consumed) to the finished
// hierarchy; put_rhs(L0) fills f and r of level 0 once the levels exist.  Returns with *unsupported
// still true when the hierarchy needs the host constructor after all.  user: A_0 is a caller's
// matrix (amg_hip_create_tensor_dev): every opt.layout is honoured, levels that do not take the
// dictionary are packed by K-SellPack with upload_mat's rule, and levels that are not bitwise
// symmetric are transposed by K-Transpose, so that no level crosses to the host.  The model
// problem's front ends keep the launches they had.  Of h: the grid of level 0 (dim 0: the flat
// index is coarsened), the semi-coarsening rule, whose automatic form takes K-AxisStrength's maxima
// and makes n_levels an upper bound, and the periodic axes, L.tper of every level.
template <class PutRhs>
amg_hip_status device_level_loop(amg_hip_solver* s, DevCsr& cur, const HierarchySpec& h, bool user, int32_t n_levels,
                                 SetupLap& lap, PutRhs&& put_rhs, bool* unsupported) {
  const int dim = h.dim;
  const bool tensor = dim != 0;
  const SemiRule* semi = h.semi;
  *unsupported = true;
  const amg_hip_options& o = s->opt;
  const bool lex = o.smoother <= AMG_HIP_SM_SOR;
  const bool cheb = o.smoother == AMG_HIP_SM_CHEBYSHEV;
  const bool line = o.smoother == AMG_HIP_SM_LINE_JACOBI;
  const bool alt = o.smoother == AMG_HIP_SM_LINE_ALT;
  const bool timing = lap.on;
  const bool try_dict = o.layout == AMG_HIP_LAYOUT_AUTO || o.layout == AMG_HIP_LAYOUT_DICT;
  s->lv.resize(n_levels);
  DevMem stats, gbound, axis_w;
  HIP_TRY(stats.alloc(sizeof(int32_t) * 2));
  if (semi && !semi->masks) HIP_TRY(axis_w.alloc(sizeof(uint64_t) * 3));
  if (cheb) HIP_TRY(gbound.alloc(sizeof(uint64_t) * 2));
  const bool prune = !o.keep_structural_zeros;
  int64_t tdims[3] = {1, 1, 1};  // tensor: the grid of the current level
  for (int a = 0; tensor && a < 3; ++a) tdims[a] = h.dims[a];
  // user: one form of a level (its rows, or its columns walked as rows) into its device layout
  // without the host: the dictionary when the layout allows it and the matrix qualifies, else
  // K-SellPack.  *done = false: the host upload has to do it.
  auto encode_dev = [&](int l, const DevCsr& M, int maxlen, DevMat* D, bool* done) -> amg_hip_status {
    *done = false;
    if (try_dict) HIP_TRY(device_dict_encode(M, prune, maxlen, D, done));
    if (*done) return AMG_HIP_OK;
    HIP_TRY(device_sell_pack(M, o.layout, prune, D, done));
    if (timing && *done)
      std::fprintf(stderr, "amg_hip device setup: level %d (%lld rows, longest row %d) -> K-SellPack (%s)\n", l,
                   (long long)M.n_rows, maxlen, D->sell ? "SELL-64" : "CSR");
    return AMG_HIP_OK;
  };
  for (int l = 0; l < n_levels; ++l) {
    Level& L = s->lv[l];
    L.n = cur.n_rows;
    L.nnz_struct = cur.nnz;
    if (tensor) {
      L.tdim = dim;
      for (int a = 0; a < 3; ++a) L.dims[a] = tdims[a];
      L.tsides = (uint32_t)o.natural_sides;
      L.tper = h.periodic;
    }
    if (tensor && l + 1 < n_levels) {  // the axes this level coarsens
      bool last = false;
      AMG_TRY(level_axis_mask(L, l, dim, semi, [&](double w[3]) -> amg_hip_status {
        HIP_TRY(launch_axis_strength(L.n, dim, L.dims, cur.rowptr(), cur.col(), cur.v(), axis_w.as<uint64_t>(), nullptr));
        HIP_TRY(hipMemcpy(w, axis_w.p, sizeof(double) * 3, hipMemcpyDeviceToHost));
        return AMG_HIP_OK;
      }, &L.tmask, &last));
      if (last) {
        n_levels = l + 1;
        s->lv.resize((size_t)n_levels);
      }
    }
    if (cheb) {  // Gershgorin bound of D^-1 A on the device CSR (K-Setup: gershgorin_kernel)
      HIP_TRY(launch_gershgorin(L.n, cur.rowptr(), cur.col(), cur.v(), gbound.as<uint64_t>(), nullptr));
      uint64_t g[2];
      HIP_TRY(hipMemcpy(g, gbound.p, sizeof(g), hipMemcpyDeviceToHost));
      if (g[1] != ~(uint64_t)0) return fail(AMG_HIP_EINVAL, cheb_zero_diag(l, (int64_t)g[1]));
      double G;
      std::memcpy(&G, &g[0], sizeof(G));
      L.cheb_lo = o.cheb_lower * G;
      L.cheb_hi = o.cheb_upper * G;
    }
    if (line) {  // stride rule and factors of T on the device CSR (K-Line setup)
      const amg_hip_status lr = line_setup_dev(l, L.n, cur.rowptr(), cur.col(), cur.v(), 0, &L.line);
      if (lr != AMG_HIP_OK) return lr;
    }
    if (alt) {  // directions of the level's grid and their factors (K-LineX and K-Line set-up)
      L.alt.set_grid(L.n, L.dims, o.cyclic_lines ? h.periodic : 0u);
      const amg_hip_status ar = alt_setup_dev(l, cur.rowptr(), cur.col(), cur.v(), &L.alt);
      if (ar != AMG_HIP_OK) return ar;
    }
    HIP_TRY(L.diag.alloc(sizeof(double) * L.n));
    HIP_TRY(hipMemset(stats.p, 0, sizeof(int32_t) * 2));
    HIP_TRY(launch_csr_inspect(L.n, cur.rowptr(), cur.col(), cur.v(), prune, stats.as<int32_t>(),
                               L.diag.as<double>(), nullptr));
    int32_t st[2];
    HIP_TRY(hipMemcpy(st, stats.p, sizeof(st), hipMemcpyDeviceToHost));
    L.symmetric = st[1] == 0;
    bool ok = false;
    if (!L.symmetric) {
      // Galerkin sums of a deep 3-D level can differ in the last bit between (i, j) and (j, i):
      // the smoothers then walk the columns of A (smoother.hpp:101-117), the residual its rows.
      // Both forms of this one level are made on the host (transpose) and uploaded; the chain
      // itself stays on the device.
      if (lex) return AMG_HIP_OK;
      bool both = false;
      if (user) {  // K-Transpose, then both forms like any level
        DevCsr csc;
        bool tr = false;
        HIP_TRY(device_transpose(cur, &csc, &tr));
        if (timing) std::fprintf(stderr, "amg_hip device setup: level %d (%lld rows) not bitwise symmetric -> K-Transpose%s\n",
                                 l, (long long)L.n, tr ? "" : " refused (a column is too long)");
        if (tr) {
          bool rows_done = false, cols_done = true;
          amg_hip_status er = encode_dev(l, cur, st[0], &L.A_rows, &rows_done);
          if (er != AMG_HIP_OK) return er;
          // the smoothers that walk the columns of A (build_solver: true Jacobi; Chebyshev and the
          // line smoother use its rows)
          if (rows_done && o.smoother == AMG_HIP_SM_JACOBI) {
            HIP_TRY(hipMemset(stats.p, 0, sizeof(int32_t) * 2));  // longest column, for the encoder
            HIP_TRY(launch_csr_inspect(L.n, csc.rowptr(), csc.col(), csc.v(), prune, stats.as<int32_t>(), nullptr,
                                       nullptr));
            int32_t st2[2];
            HIP_TRY(hipMemcpy(st2, stats.p, sizeof(st2), hipMemcpyDeviceToHost));
            er = encode_dev(l, csc, st2[0], &L.A_cols_own, &cols_done);
            if (er != AMG_HIP_OK) return er;
          }
          both = rows_done && cols_done;
          if (both) {
            L.A_dev = std::move(csc);  // CSC(A): what ensure_host_matrix downloads
          } else {
            L.A_rows = DevMat();
            L.A_cols_own = DevMat();
          }
        }
      }
      if (!both) {
      if (timing) std::fprintf(stderr, "amg_hip device setup: level %d (%lld rows) not bitwise symmetric -> rows and columns uploaded separately\n",
                               l, (long long)L.n);
      Sparse H;
      HIP_TRY(download_csr(cur, &H));
      HIP_TRY(upload_mat_pruned(H, o.layout, prune, &L.A_rows));       // H = CSR(A)
      L.A_csc = transpose(H);                                           // CSC(A)
      HIP_TRY(upload_mat_pruned(L.A_csc, o.layout, prune, &L.A_cols_own));
      }
      ok = true;
    } else if (user) {
      const amg_hip_status er = encode_dev(l, cur, st[0], &L.A_rows, &ok);
      if (er != AMG_HIP_OK) return er;
    } else {
      HIP_TRY(device_dict_encode(cur, prune, st[0], &L.A_rows, &ok));
    }
    if (!ok) {
      // this level does not qualify for the dictionary (rows of more than 16 entries on the
      // deep 3-D levels, more than 255 pairs): its CSR arrays go to the host once and take
      // the general upload (SELL-64 / CSR panels); the chain itself stays on the device
      if (timing) std::fprintf(stderr, "amg_hip device setup: level %d (%lld rows, longest row %d) -> panel layout\n",
                               l, (long long)L.n, (int)st[0]);
      L.A_dev.n_rows = 0;
      Sparse H;
      HIP_TRY(download_csr(cur, &H));
      HIP_TRY(upload_mat_pruned(H, user ? o.layout : AMG_HIP_LAYOUT_SELL, prune, &L.A_rows));
      L.A_csc = std::move(H);  // symmetric: the CSR arrays are the CSC arrays
    }
    if (o.smoother != AMG_HIP_SM_JACOBI) L.diag.release();
    AMG_TRY(alloc_level_vectors(L, cheb));
    // K-GS-scan on every smoothed level, or the host path
    if (lex && (l + 1 < n_levels || o.keep_residual) && !gs_scan_params(L.A_rows, &L.scan_C, &L.scan_ring))
      return AMG_HIP_OK;
    if (l + 1 == n_levels) {
      if (L.A_csc.ptr.empty() && L.A_dev.n_rows == 0) L.A_dev = std::move(cur);
      break;
    }
    DevCsr next;
    if (tensor) {  // every coarsened axis m -> floor(m / 2), matrix-free transfers, K-TensorGalerkin
      const std::string e = level_mask_error(l, dim, L.dims, L.tmask, semi != nullptr);
      if (!e.empty()) return fail(AMG_HIP_EINVAL, e);
      tensor_coarse_dims(dim, L.dims, L.tmask, tdims);
      L.tensor = true;
      L.tensor_stencil = true;  // o.stencil_transfers is set and N < 2^28
      L.n_coarse = tdims[0] * tdims[1] * tdims[2];
      const bool opdep = semi && semi->opdep;
      std::chrono::steady_clock::time_point tk[3];
      if (opdep) {  // one axis, K-AxisWeights from this level's rows into the transfers' own array; kind 3
        L.tensor_stencil = false;
        L.axis_stencil = true;
        for (L.axis = 0; !((L.tmask >> L.axis) & 1u); ++L.axis) {}
        HIP_TRY(L.axis_W_dev.alloc(sizeof(double) * 2 * (L.n - L.n_coarse)));
        const int32_t none = INT32_MAX;
        int32_t first_bad = none;
        HIP_TRY(hipMemcpy(stats.p, &none, sizeof(int32_t), hipMemcpyHostToDevice));
        if (timing) tk[0] = std::chrono::steady_clock::now();  // the copy above has synchronised
        HIP_TRY(launch_axis_weights(dim, L.dims, L.axis, L.tper, cur.rowptr(), cur.col(), cur.v(),
                                    L.axis_W_dev.as<double>(), stats.as<int32_t>(), nullptr));
        HIP_TRY(hipMemcpy(&first_bad, stats.p, sizeof(int32_t), hipMemcpyDeviceToHost));
        if (timing) tk[1] = std::chrono::steady_clock::now();
        if (first_bad != none) {  // that one row to the host, worded by the host constructor's code
          int32_t rp[2];
          HIP_TRY(hipMemcpy(rp, cur.rowptr() + first_bad, sizeof(rp), hipMemcpyDeviceToHost));
          std::vector<int32_t> ci((size_t)std::max(rp[1] - rp[0], 1));
          std::vector<double> cv(ci.size());
          if (rp[1] > rp[0]) {
            HIP_TRY(hipMemcpy(ci.data(), cur.col() + rp[0], sizeof(int32_t) * (rp[1] - rp[0]), hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(cv.data(), cur.v() + rp[0], sizeof(double) * (rp[1] - rp[0]), hipMemcpyDeviceToHost));
          }
          const int64_t stride = L.axis == 0 ? 1 : (L.axis == 1 ? L.dims[0] : L.dims[0] * L.dims[1]);
          double w2[2];
          std::string we = axis_opdep_row(first_bad, ci.data(), cv.data(), rp[1] - rp[0], stride, L.dims[L.axis], L.axis, w2,
                                          L.axis_periodic());
          if (we.empty()) we = "row " + std::to_string(first_bad) + ": refused by K-AxisWeights";
          return fail(AMG_HIP_EINVAL, std::string(semi->opdep_who) + "level " + std::to_string(l) + ": " + we);
        }
      }
      bool ok_g = false;
      const hipError_t ge = device_tensor_galerkin(cur, dim, L.dims, L.tmask, L.tsides, L.tper, L.n_coarse, &next, &ok_g,
                                                   opdep ? L.axis : -1, L.axis_W_dev.as<double>());
      if (opdep && timing && ge == hipSuccess && ok_g) {
        (void)hipDeviceSynchronize();
        tk[2] = std::chrono::steady_clock::now();
        std::fprintf(stderr, "amg_hip device setup: level %d (%lld rows, axis %c) K-AxisWeights %.3f ms, K-AxisGalerkin %.3f ms\n",
                     l, (long long)L.n, "xyz"[L.axis], 1e3 * std::chrono::duration<double>(tk[1] - tk[0]).count(),
                     1e3 * std::chrono::duration<double>(tk[2] - tk[1]).count());
      }
      if (ge == hipErrorInvalidValue || (ge == hipSuccess && !ok_g)) {
        if (timing) std::fprintf(stderr, "amg_hip device setup: Galerkin product of level %d exceeds %s -> host path\n", l,
                                 ge == hipSuccess ? "the kernel's columns per coarse row" : "int32 indexing");
        return AMG_HIP_OK;
      }
      HIP_TRY(ge);
    } else {
    const int64_t n_H = coarse_dofs(L.n);  // multigrid.hpp:214
    if (n_H < 1)
      return fail(AMG_HIP_EINVAL, "level " + std::to_string(l + 1) +
                                      " would have no degrees of freedom; reduce `n_levels`");
    L.lazy_linear = true;
    L.n_coarse = n_H;
    L.linear = true;
    {
      const hipError_t ge = device_galerkin(cur, n_H, &next, nullptr);
      if (ge == hipErrorInvalidValue) {  // an intermediate product beyond int32 indices: host path
        if (timing) std::fprintf(stderr, "amg_hip device setup: Galerkin product of level %d exceeds int32 indexing -> host path\n", l);
        return AMG_HIP_OK;
      }
      HIP_TRY(ge);
    }
    }
    if (L.A_csc.ptr.empty() && L.A_dev.n_rows == 0) L.A_dev = std::move(cur);
    cur = std::move(next);
  }
  lap("hierarchy");
  if (o.singular && n_levels < 2) return fail(AMG_HIP_EINVAL, SINGULAR_ONE_LEVEL);
  AMG_TRY(put_rhs(s->lv[0]));
  lap("rhs");
  if (!o.window) HIP_TRY(s->lv[n_levels - 1].ensure_host_matrix());  // for the coarsest factor
  AMG_TRY(finish_device_solver(s, [&] { lap("coarse factor"); }));
  s->device_setup = true;
  *unsupported = false;
  return AMG_HIP_OK;
}

// Front end of the model problem: AMG::Multigrid's constructor (multigrid.hpp:151-244) for A = Grid::laplacian(n), b =
// Grid::rhs(n) without host matrices: generator, Galerkin chain, dictionary encoder, diagonal
// and symmetry check all run on the device; only b (n^dim exp() calls, kept on the host so that
// the bits are libm's, like the reference's) and the coarsest operator (factored on the host)
// cross PCIe.  *unsupported = true: the options need host structures (exact lexicographic
// schedules, multicolouring, non-dictionary layouts): the caller takes the host path instead.
// [unit0, unit1): the grid lines (2-D) / x-y planes (3-D) of a window solver, else unit1 < 0.
amg_hip_status build_poisson_device(int dim, int64_t n, int32_t n_levels, const amg_hip_options& o,
                                    amg_hip_solver** out, bool* unsupported, int64_t unit0 = 0,
                                    int64_t unit1 = -1, bool tensor = false) {
  *unsupported = true;
  if (unit1 < 0) { unit0 = 0; unit1 = n; }
  const int64_t n_last = unit1 - unit0;
  const int64_t unit_rows = dim == 3 ? n * n : n;
  const int64_t N = unit_rows * n_last;
  const bool lex = o.smoother <= AMG_HIP_SM_SOR;
  if (o.host_only || o.host_galerkin || !o.stencil_transfers || o.fuse_prolong ||
      (o.layout != AMG_HIP_LAYOUT_AUTO && o.layout != AMG_HIP_LAYOUT_DICT) ||
      o.smoother == AMG_HIP_SM_MULTICOLOR_GS || (lex && (o.exact_gs || N <= GS_SCAN_MIN_ROWS)) ||
      n_levels < 2 || N >= ((int64_t)1 << 28))
    return AMG_HIP_OK;
  // full coarsening: the lexicographic and the line smoothers build through the host constructor
  if (tensor && (lex || o.smoother == AMG_HIP_SM_LINE_JACOBI || o.smoother == AMG_HIP_SM_LINE_ALT)) return AMG_HIP_OK;
  // a bad option (and the alternating line smoother without a grid): the host path words the error
  if (smoother_options_error(o, tensor ? dim : 0, n_levels) != AMG_HIP_OK) return AMG_HIP_OK;
  std::unique_ptr<amg_hip_solver> s;
  AMG_TRY(device_setup_begin(o, &s));
  SetupLap lap;
  // b on the host threads while the device builds the hierarchy
  std::vector<double> b((size_t)N);
  std::thread rhs_thread([&] { rhs_threads(dim, n, b.data(), host_threads(), unit0 * unit_rows, unit1 * unit_rows); });
  struct Joiner { std::thread& t; ~Joiner() { if (t.joinable()) t.join(); } } joiner{rhs_thread};
  // A_0 (grid.hpp:88-98)
  DevCsr cur;
  {
    DevMem cnt, bsum, total;
    HIP_TRY(cnt.alloc(sizeof(int32_t) * (N + 1)));
    HIP_TRY(bsum.alloc(sizeof(int64_t) * ((N + 1023) / 1024 + 1)));
    HIP_TRY(total.alloc(sizeof(int64_t)));
    HIP_TRY(launch_laplacian_count(dim, n, n_last, N, cnt.as<int32_t>(), nullptr));
    HIP_TRY(cur.ptr.alloc(sizeof(int32_t) * (N + 1)));
    HIP_TRY(launch_exclusive_scan(N, cnt.as<int32_t>(), cur.ptr.as<int32_t>(), bsum.as<int64_t>(),
                                  total.as<int64_t>(), nullptr));
    int64_t nnz = 0;
    HIP_TRY(hipMemcpy(&nnz, total.p, sizeof(int64_t), hipMemcpyDeviceToHost));
    if (nnz >= ((int64_t)1 << 31) - 1) return AMG_HIP_OK;
    HIP_TRY(cur.idx.alloc(sizeof(int32_t) * nnz));
    HIP_TRY(cur.val.alloc(sizeof(double) * nnz));
    const double h = 2.0 / (double)(n + 1), hh = h * h;
    const double off = 1.0 / hh, dg = -2.0 / hh;
    double diag = dg + dg;
    if (dim == 3) diag = diag + dg;
    HIP_TRY(launch_laplacian_fill(dim, n, n_last, N, cur.ptr.as<int32_t>(), cur.idx.as<int32_t>(),
                                  cur.val.as<double>(), off, diag, nullptr));
    cur.n_rows = cur.n_cols = N;
    cur.nnz = nnz;
  }
  lap("generator");
  const int64_t dims0[3] = {n, n, dim == 3 ? n : 1};
  auto put_rhs = [&](Level& L0) -> amg_hip_status {
    joiner.t.join();
    HIP_TRY(hipMemcpy(L0.f.p, b.data(), sizeof(double) * N, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(L0.r.p, b.data(), sizeof(double) * N, hipMemcpyHostToDevice));  // b - A*0
    return AMG_HIP_OK;
  };
  HierarchySpec h;
  if (tensor) {
    h.dim = dim;
    h.dims = dims0;
  }
  const amg_hip_status r = device_level_loop(s.get(), cur, h, false, n_levels, lap, put_rhs, unsupported);
  if (r != AMG_HIP_OK || *unsupported) return r;
  *out = s.release();
  return AMG_HIP_OK;
}

// ---- helpers for the stand-alone host-array entry points ---------------------
struct Scoped {
  hipStream_t st = nullptr;
  ~Scoped() { if (st) (void)hipStreamDestroy(st); }
};

// Grid::rhs on several host threads (the values are libm's exp(), as in the reference);
// entries [d0, d1) of the right-hand side into b[0 .. d1 - d0) (d1 < 0: all)
void rhs_threads(int dim, int64_t n, double* b, int nt, int64_t d0, int64_t d1) {
  int64_t N = n * n;
  if (dim == 3) N *= n;
  if (d1 < 0) { d0 = 0; d1 = N; }
  const int64_t M = d1 - d0;
  if (nt <= 1 || M < (1 << 18)) {
    rhs_range(dim, n, b - d0, d0, d1);
    return;
  }
  std::vector<std::thread> th;
  for (int t = 0; t < nt; ++t)
    th.emplace_back([=] { rhs_range(dim, n, b - d0, d0 + M * t / nt, d0 + M * (t + 1) / nt); });
  for (auto& x : th) x.join();
}

amg_hip_status need_device() {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(AMG_HIP_EHIP, "no HIP device available (this library has no CPU fallback)");
  return AMG_HIP_OK;
}

// ---- block (multi-right-hand-side) cycle ---------------------------------------
// The same V-cycle as enqueue_vcycle_body on kp columns at once, with plain launches of the K-Block
// kernels on CSR: per (row, column) every kernel does the operations of the single-vector path's
// unfused form in the same order, and the fusions of that path are bit-neutral, so column j ends
// with the bits of vcycle() on column j ("Block cycle").
const char* block_smoother_name(int32_t sm) {
  switch (sm) {
    case AMG_HIP_SM_SPGS: return "SparseGaussSeidel (AMG_HIP_SM_SPGS)";
    case AMG_HIP_SM_REF_JACOBI: return "AMG::Jacobi (AMG_HIP_SM_REF_JACOBI)";
    case AMG_HIP_SM_SOR: return "SOR (AMG_HIP_SM_SOR)";
    case AMG_HIP_SM_MULTICOLOR_GS: return "multicolour Gauss-Seidel (AMG_HIP_SM_MULTICOLOR_GS)";
    case AMG_HIP_SM_LINE_JACOBI: return "line Jacobi (AMG_HIP_SM_LINE_JACOBI)";
    case AMG_HIP_SM_LINE_ALT: return "alternating line Jacobi (AMG_HIP_SM_LINE_ALT)";
  }
  return "unknown";
}
bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }
int block_kp(int32_t k) {
  int kp = 1;
  while (kp < k) kp *= 2;
  return kp;
}
// steps 2 and 3 of the argument checks (include/amg_hip.h: amg_hip_block_vcycles)
amg_hip_status block_supported(amg_hip_solver* s) {
  if (s->opt.window)
    return fail(AMG_HIP_EUNSUPPORTED, "block cycles: a window solver (opt.window) is not supported");
  const bool line = s->opt.smoother == AMG_HIP_SM_LINE_JACOBI || s->opt.smoother == AMG_HIP_SM_LINE_ALT;
  if (s->opt.smoother != AMG_HIP_SM_JACOBI && s->opt.smoother != AMG_HIP_SM_CHEBYSHEV && !(g_block_lines && line))
    return fail(AMG_HIP_EUNSUPPORTED,
                std::string("block cycles: the smoother ") + block_smoother_name(s->opt.smoother) +
                    (g_block_lines ? " is not supported (true Jacobi, Chebyshev, AMG_HIP_SM_LINE_JACOBI and "
                                     "AMG_HIP_SM_LINE_ALT are)"
                                   : " is not supported (true Jacobi and Chebyshev are)"));
  return set_device(s);
}
bool has_exact_zero(const Sparse& M) {
  for (double v : M.val)
    if (v == 0.0) return true;
  return false;
}
double csr_bytes(const DevCsr& M) { return 12.0 * (double)M.nnz + 4.0 * (double)(M.n_rows + 1); }

// CSR(P), CSR(R) of a level whose transfers run as K-AxisRestrict / K-AxisProlong: the float and the
// block cycles take their CSR kernels on such a level
amg_hip_status ensure_axis_rows(Level& L) {
  if (!L.axis_stencil || L.P_rows.n_rows != 0) return AMG_HIP_OK;
  HIP_TRY(L.ensure_axis_weights());  // a level built on the device: its host operators are made here
  HIP_TRY(upload_csr(transpose(L.P()), &L.P_rows));
  HIP_TRY(upload_csr(transpose(L.R()), &L.R_rows));
  return AMG_HIP_OK;
}

// the CSR copies (once) and the panels for pitch kp (again only when kp grows)
amg_hip_status ensure_block(amg_hip_solver* s, int kp) {
  Block& B = s->blk;
  const int nl = (int)s->lv.size();
  const bool prune = !s->opt.keep_structural_zeros;
  if (!B.mats) {
    B.lv.clear();
    B.lv.resize((size_t)nl);
    for (int l = 0; l < nl; ++l) {
      Level& L = s->lv[l];
      BlockLevel& Q = B.lv[(size_t)l];
      if (L.tensor_stencil && l + 1 < nl && L.P_rows.n_rows == 0) {
        // the block transfers of a full-coarsening level are the CSR kernels (same bits)
        HIP_TRY(upload_csr(transpose(L.P()), &L.P_rows));
        HIP_TRY(upload_csr(transpose(L.R()), &L.R_rows));
        L.P_csc = Sparse();
        L.R_csc = Sparse();
      }
      AMG_TRY(ensure_axis_rows(L));
      if (l + 1 == nl && l > 0) continue;  // the coarsest level only takes the direct solve
      // the entry set of the device matrices: exact zeros dropped unless keep_structural_zeros,
      // ascending column order (A_rows is plain CSR already when its layout is)
      if (!L.A_rows.dict && !L.A_rows.sell) {
        Q.rows = &L.A_rows.csr;
      } else {
        HIP_TRY(L.ensure_host_matrix());
        const Sparse rows = L.symmetric ? L.A_csc : transpose(L.A_csc);  // CSR(A)
        HIP_TRY(upload_csr(prune && has_exact_zero(rows) ? without_exact_zeros(rows) : rows, &Q.rows_own));
        Q.rows = &Q.rows_own;
      }
      Q.cols = Q.rows;
      if (!L.symmetric && s->opt.smoother == AMG_HIP_SM_JACOBI) {
        const DevMat& Ac = L.A_cols();
        if (!Ac.dict && !Ac.sell) {
          Q.cols = &Ac.csr;
        } else {
          HIP_TRY(L.ensure_host_matrix());
          HIP_TRY(upload_csr(prune && has_exact_zero(L.A_csc) ? without_exact_zeros(L.A_csc) : L.A_csc, &Q.cols_own));
          Q.cols = &Q.cols_own;
        }
      }
    }
    B.mats = true;
  }
  if (kp <= B.kp_alloc) return AMG_HIP_OK;
  B.reset_graphs();  // their pointers are about to change
  const bool cheb = s->opt.smoother == AMG_HIP_SM_CHEBYSHEV;
  const bool line = s->opt.smoother == AMG_HIP_SM_LINE_JACOBI || s->opt.smoother == AMG_HIP_SM_LINE_ALT;
  for (int l = 0; l < nl; ++l) {
    const size_t bytes = sizeof(double) * (size_t)s->lv[l].n * (size_t)kp;
    BlockLevel& Q = B.lv[(size_t)l];
    HIP_TRY(Q.U.alloc(bytes));
    HIP_TRY(Q.F.alloc(bytes));
    if (l + 1 < nl || l == 0) {
      HIP_TRY(Q.R.alloc(bytes));
      HIP_TRY(Q.T.alloc(bytes));
      if (cheb) HIP_TRY(Q.D.alloc(bytes));
      if (line && l + 1 < nl) HIP_TRY(Q.Y.alloc(bytes));
    }
  }
  const size_t cb = sizeof(double) * (size_t)s->lv[nl - 1].n * (size_t)kp;
  HIP_TRY(B.cf.alloc(cb));
  HIP_TRY(B.cy.alloc(cb));
  HIP_TRY(B.cx.alloc(cb));
  B.px.release();  // PCG panels: allocated at the first block_pcg for this pitch
  B.pp.release();
  B.pq.release();
  B.pb.release();
  if (!B.part.p) {
    HIP_TRY(B.part.alloc(sizeof(double) * 1024 * BLOCK_K_MAX));
    HIP_TRY(B.dots.alloc(sizeof(double) * 6 * BLOCK_K_MAX));
    HIP_TRY(B.act.alloc(sizeof(int32_t) * BLOCK_K_MAX));
  }
  B.kp_alloc = kp;
  return AMG_HIP_OK;
}

#define STEP_TRY(X, expr)            \
  do {                               \
    if ((X).launch) HIP_TRY(expr);   \
  } while (0)

// multigrid.hpp:263-305 as one plain launch per step on a single stream (enqueue_vcycle_body's order:
// down-legs, coarsest solve, up-legs).  S: the steps of the block or of the float cycle.
template <typename Steps>
amg_hip_status walk_vcycle(int nl, Steps&& S) {
  for (int l = 0; l + 1 < nl; ++l) {
    AMG_TRY(S.smooth(l, false));  // :268
    AMG_TRY(S.residual(l));       // :272-274
    AMG_TRY(S.restriction(l));       // :278 + :281-282
  }
  AMG_TRY(S.coarse());            // :287-288
  for (int l = nl - 2; l >= 0; --l) {  // :291
    AMG_TRY(S.prolong(l));        // :294-296
    AMG_TRY(S.smooth(l, true));   // :300
  }
  return AMG_HIP_OK;
}

// The steps of the block cycle on the panels of pitch kp.
struct BlockSteps {
  amg_hip_solver* s;
  int kp;
  StepCtx& X;

  // K-Line on the panels (LineOnDev::solve_bytes with the factors counted once: dl, ip, cp, v, w of every
  // row; per column 40 B on an interior and 56 B on a separator row)
  void count_line(const LineOnDev& D) {
    const int64_t sep = D.separators();
    X.count(40.0 * (double)D.n, 40.0 * (double)(D.n - sep) + 56.0 * (double)sep);
  }
  // the bytes of sub-sweep d of AMG_HIP_SM_LINE_ALT on the panels, after its residual
  void count_alt(const AltOnDev& D, int d) {
    if (D.cyclic(d)) {
      // p, then den, gamma, beta of every line once; r in and the two ends of r out per column
      const double lines = (double)(D.n / D.len[d]);
      X.count(8.0 * (double)D.n + 24.0 * lines, 8.0 * (double)D.n + 16.0 * lines);
    }
    if (D.along_x(d)) X.count(24.0 * (double)D.n, 40.0 * (double)D.n);  // dl, ip, cp; r, y, y, u, u
    else count_line(D.yz[D.yz_of(d)]);
  }

  // the smoothing of one level (enqueue_smooth's plain launches): U -> T -> U ..., home after an odd count;
  // the line smoothers update U in place (reverse: the up-leg, AMG_HIP_SM_LINE_ALT's directions descend)
  amg_hip_status smooth(int l, bool reverse) {
    Level& L = s->lv[l];
    BlockLevel& Q = s->blk.lv[(size_t)l];
    const double n = (double)L.n;
    double* F = Q.F.as<double>();
    if (s->opt.smoother == AMG_HIP_SM_LINE_JACOBI || s->opt.smoother == AMG_HIP_SM_LINE_ALT) {
      const DevCsr& A = *Q.rows;
      const bool alt = s->opt.smoother == AMG_HIP_SM_LINE_ALT;
      // a sub-sweep: T = F - A U, then the line solve updates U in place (Y: K-Line's scratch panel)
      return line_subsweeps(s->opt.smoother_iters, line_dirs(s->opt.smoother, L.alt), reverse, [&](int d) {
        STEP_TRY(X, launch_block_csr(CSR_RESID, kp, L.n, A.rowptr(), A.col(), A.v(), Q.U.as<double>(), F,
                                     Q.T.as<double>(), 1.0, X.st));
        X.count(csr_bytes(A), 24.0 * n);  // matrix; u, f, r
        STEP_TRY(X, alt ? launch_alt_dir(L.alt, d, kp, Q.T.as<double>(), Q.Y.as<double>(), Q.U.as<double>(),
                                         s->opt.omega, X.st)
                        : launch_line_dir<double>(L.line.ref(), nullptr, nullptr, kp, Q.T.as<double>(),
                                                  Q.Y.as<double>(), Q.U.as<double>(), s->opt.omega, X.st));
        if (alt) count_alt(L.alt, d);
        else count_line(L.line);
        return AMG_HIP_OK;
      });
    }
    auto copy_home = [&] {
      STEP_TRY(X, hipMemcpyAsync(Q.U.p, Q.T.p, sizeof(double) * (size_t)L.n * (size_t)kp, hipMemcpyDeviceToDevice,
                                 X.st));
      X.count(0.0, 16.0 * n);
      return AMG_HIP_OK;
    };
    if (s->opt.smoother == AMG_HIP_SM_JACOBI) {
      const DevCsr& A = *Q.cols;
      return ping_pong(s->opt.smoother_iters, Q.U.as<double>(), Q.T.as<double>(), [&](int64_t, double* a, double* b) {
        STEP_TRY(X, launch_block_csr(CSR_JACOBI, kp, L.n, A.rowptr(), A.col(), A.v(), a, F, b, s->opt.omega, X.st));
        X.count(csr_bytes(A), 24.0 * n);  // matrix; x, f, out
        return AMG_HIP_OK;
      }, copy_home);
    }
    const DevCsr& A = *Q.rows;
    return cheb_steps(L.cheb_lo, L.cheb_hi, s->opt.smoother_iters, s->opt.cheb_degree, Q.U.as<double>(),
                      Q.T.as<double>(), [&](double alpha, double beta, bool first, bool last, double* a, double* b) {
      const ChebStep c{Q.D.as<double>(), alpha, beta, first, last};
      STEP_TRY(X, launch_block_csr_cheb(kp, L.n, A.rowptr(), A.col(), A.v(), a, F, b, c, X.st));
      X.count(csr_bytes(A), 24.0 * n + (first ? 0.0 : 8.0 * n) + (last ? 0.0 : 8.0 * n));
      return AMG_HIP_OK;
    }, copy_home);
  }

  // R_l = F_l - A_l U_l
  amg_hip_status residual(int l) {
    Level& L = s->lv[l];
    BlockLevel& Q = s->blk.lv[(size_t)l];
    const DevCsr& A = *Q.rows;
    STEP_TRY(X, launch_block_csr(CSR_RESID, kp, L.n, A.rowptr(), A.col(), A.v(), Q.U.as<double>(), Q.F.as<double>(),
                                 Q.R.as<double>(), 1.0, X.st));
    X.count(csr_bytes(A), 24.0 * (double)L.n);
    return AMG_HIP_OK;
  }

  // U_{l+1} = 0, F_{l+1} = R_l R_l
  amg_hip_status restriction(int l) {
    Level& L = s->lv[l];
    Level& C = s->lv[l + 1];
    BlockLevel& Q = s->blk.lv[(size_t)l];
    BlockLevel& QC = s->blk.lv[(size_t)l + 1];
    if (L.linear && s->opt.stencil_transfers) {
      STEP_TRY(X, launch_block_restrict(kp, L.n, C.n, Q.R.as<double>(), QC.F.as<double>(), QC.U.as<double>(), X.st));
      X.count(0.0, 8.0 * (double)L.n + 16.0 * (double)C.n);
    } else {
      STEP_TRY(X, hipMemsetAsync(QC.U.p, 0, sizeof(double) * (size_t)C.n * (size_t)kp, X.st));
      const DevCsr& R = L.R_rows;
      STEP_TRY(X, launch_block_csr(CSR_SPMV, kp, R.n_rows, R.rowptr(), R.col(), R.v(), Q.R.as<double>(), nullptr,
                                   QC.F.as<double>(), 1.0, X.st));
      X.count(csr_bytes(R), 8.0 * (double)L.n + 16.0 * (double)C.n);
    }
    return AMG_HIP_OK;
  }

  // the coarsest system on kp contiguous columns: the one-wave kinds solve every column in one launch
  amg_hip_status coarse() {
    Block& B = s->blk;
    Level& C = s->lv.back();
    BlockLevel& QC = B.lv.back();
    const CoarseOnDev& K = s->coarse;
    STEP_TRY(X, launch_block_columns(kp, C.n, QC.F.as<double>(), B.cf.as<double>(), true, X.st));
    STEP_TRY(X, launch_coarse(K, B.cf.as<double>(), B.cy.as<double>(), B.cx.as<double>(), X.st, 0, nullptr, nullptr,
                              kp, C.n));
    const double factor = 16.0 * (double)C.n * (double)std::max<int64_t>(K.w, 1);
    if (K.kind == COARSE_SPIKE) X.count(0.0, factor);  // one launch per column
    else X.count(factor, 0.0);
    STEP_TRY(X, launch_block_columns(kp, C.n, B.cx.as<double>(), QC.U.as<double>(), false, X.st));
    // f and u of the solve; the two reorderings read and write each once
    X.count(0.0, 24.0 * (double)C.n + 32.0 * (double)C.n);
    return AMG_HIP_OK;
  }

  // U_l = U_l + P_l U_{l+1}
  amg_hip_status prolong(int l) {
    Level& L = s->lv[l];
    Level& C = s->lv[l + 1];
    BlockLevel& Q = s->blk.lv[(size_t)l];
    BlockLevel& QC = s->blk.lv[(size_t)l + 1];
    if (L.linear && s->opt.stencil_transfers) {
      STEP_TRY(X, launch_block_prolong_add(kp, L.n, C.n, QC.U.as<double>(), Q.U.as<double>(), X.st));
      X.count(0.0, 8.0 * (double)C.n + 16.0 * (double)L.n);
    } else {
      const DevCsr& P = L.P_rows;
      STEP_TRY(X, launch_block_csr(CSR_SPMV_ADD, kp, P.n_rows, P.rowptr(), P.col(), P.v(), QC.U.as<double>(),
                                   Q.U.as<double>(), Q.U.as<double>(), 1.0, X.st));
      X.count(csr_bytes(P), 8.0 * (double)C.n + 16.0 * (double)L.n);
    }
    return AMG_HIP_OK;
  }
};

// one block cycle on the panels of pitch kp
amg_hip_status enqueue_block_vcycle(amg_hip_solver* s, int kp, StepCtx& X) {
  return walk_vcycle((int)s->lv.size(), BlockSteps{s, kp, X});
}

int log2i(int kp) { return __builtin_ctz((unsigned)kp); }

// n block cycles on the panels of level 0 (their pitch is kp): the captured graph of this kp, or
// the same enqueue eagerly (use_graph = 0)
amg_hip_status run_block_cycles(amg_hip_solver* s, int kp, int32_t n) {
  return replay_or_enqueue(s->opt.use_graph, s->blk.graph[log2i(kp)], s->stream,
                           [s, kp] {
                             StepCtx X{s->stream};
                             return enqueue_block_vcycle(s, kp, X);
                           }, n);
}

// out[j] (host, j < kp) = sum_i x[i, j] (y null) or x[i, j] y[i, j] over level 0's rows
amg_hip_status block_sums_to_host(amg_hip_solver* s, int kp, const double* x, const double* y, double* out) {
  double* d = s->blk.dots.as<double>() + 3 * BLOCK_K_MAX;  // past block_pcg's rz, pq, rz_new
  HIP_TRY(launch_block_sum(kp, s->lv[0].n, x, y, d, s->blk.part.as<double>(), s->stream));
  HIP_TRY(hipMemcpyAsync(out, d, sizeof(double) * (size_t)kp, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return AMG_HIP_OK;
}

// ---- fp32 cycle (single-precision preconditioner) -------------------------------
// multigrid.hpp:263-305 from a zero guess on float vectors with the K-F32 kernels, one plain launch
// per step on the solver's stream (enqueue_block_vcycle's order).  Not bitwise against the double
// cycle: a zero-filled u_H plus the normal sweep stands for the from-zero sweep, and the coarsest
// system is solved in double with the solver's factor ("Single-precision preconditioner").
// steps 3 to 5 of the argument checks (include/amg_hip.h), then the device
amg_hip_status f32_supported(amg_hip_solver* s) {
  if (s->opt.window)
    return fail(AMG_HIP_EUNSUPPORTED, "single-precision cycle: a window solver (opt.window) is not supported");
  const bool line = s->opt.smoother == AMG_HIP_SM_LINE_JACOBI || s->opt.smoother == AMG_HIP_SM_LINE_ALT;
  if (s->opt.smoother != AMG_HIP_SM_JACOBI && s->opt.smoother != AMG_HIP_SM_CHEBYSHEV && !(g_f32_lines && line))
    return fail(AMG_HIP_EUNSUPPORTED,
                std::string("single-precision cycle: the smoother ") + block_smoother_name(s->opt.smoother) +
                    (g_f32_lines ? " is not supported (true Jacobi, Chebyshev, AMG_HIP_SM_LINE_JACOBI and "
                                   "AMG_HIP_SM_LINE_ALT are)"
                                 : " is not supported (true Jacobi and Chebyshev are)"));
  if (s->lv.size() < 2)
    return fail(AMG_HIP_EUNSUPPORTED, "single-precision cycle: a one-level solver has no cycle (the direct solve "
                                      "stays in double); use amg_hip_apply");
  return set_device(s);
}

amg_hip_status f32_copy_values(const DevMat& A, F32Mat* M, hipStream_t st) {
  M->src = &A;
  // a dictionary matrix has no per-entry values: its float form is the pair table alone
  const double* src = A.dict ? A.dval.as<double>() : A.sell ? A.sval.as<double>() : A.csr.v();
  const int64_t count = A.dict ? A.dict_ntab : A.sell ? A.slots : A.csr.nnz;
  HIP_TRY(M->val.alloc(sizeof(float) * (size_t)std::max<int64_t>(count, 1)));
  HIP_TRY(launch_to_f32(count, src, M->val.as<float>(), st));
  return AMG_HIP_OK;
}

// a float copy of `count` doubles of a factor array, made on the device
amg_hip_status f32_copy_array(const DevMem& src, int64_t count, DevMem* dst, hipStream_t st) {
  HIP_TRY(dst->alloc(sizeof(float) * (size_t)std::max<int64_t>(count, 1)));
  HIP_TRY(launch_to_f32(count, src.as<double>(), dst->as<float>(), st));
  return AMG_HIP_OK;
}
amg_hip_status f32_copy_line(const LineOnDev& D, F32Line* Q, hipStream_t st) {
  amg_hip_status r;
  const DevMem* src[5] = {&D.dl, &D.ip, &D.cp, &D.v, &D.w};
  DevMem* dst[5] = {&Q->dl, &Q->ip, &Q->cp, &Q->v, &Q->w};
  for (int k = 0; k < 5; ++k)
    if ((r = f32_copy_array(*src[k], D.n, dst[k], st)) != AMG_HIP_OK) return r;
  HIP_TRY(Q->y.alloc(sizeof(float) * (size_t)D.n));
  return AMG_HIP_OK;
}
// the float factors of a level's line smoother: copies of the double ones, no float elimination
amg_hip_status f32_copy_line_factors(const amg_hip_solver* s, const Level& L, F32Level* Q, hipStream_t st) {
  if (s->opt.smoother == AMG_HIP_SM_LINE_JACOBI) return f32_copy_line(L.line, &Q->line, st);
  const AltOnDev& D = L.alt;
  amg_hip_status r;
  if (D.n_dir == 0) return f32_copy_line(D.yz[0], &Q->yz[0], st);
  for (int d = 0; d < D.n_dir; ++d) {
    const int a = D.axis[d];
    if (a == 0) {
      if ((r = f32_copy_array(D.xdl, D.n, &Q->xdl, st)) != AMG_HIP_OK) return r;
      if ((r = f32_copy_array(D.xip, D.n, &Q->xip, st)) != AMG_HIP_OK) return r;
      if ((r = f32_copy_array(D.xcp, D.n, &Q->xcp, st)) != AMG_HIP_OK) return r;
    } else if ((r = f32_copy_line(D.yz[a - 1], &Q->yz[a - 1], st)) != AMG_HIP_OK) {
      return r;
    }
    if (D.cyc[d]) {
      if ((r = f32_copy_array(D.seam_p[d], D.n, &Q->seam_p[d], st)) != AMG_HIP_OK) return r;
      if ((r = f32_copy_array(D.seam_coef[d], 3 * (D.n / D.len[d]), &Q->seam_coef[d], st)) != AMG_HIP_OK) return r;
    }
  }
  return AMG_HIP_OK;
}

amg_hip_status ensure_f32(amg_hip_solver* s) {
  F32& F = s->f32;
  if (F.ready) return AMG_HIP_OK;
  const int nl = (int)s->lv.size();
  const bool jac = s->opt.smoother == AMG_HIP_SM_JACOBI;
  const bool line = s->opt.smoother == AMG_HIP_SM_LINE_JACOBI || s->opt.smoother == AMG_HIP_SM_LINE_ALT;
  // g_f32_dict is read here and nowhere else: nothing is cached on a refusal, so a solver refused with the
  // switch off is accepted once it is on, and a solver whose copies exist (F.ready) never comes back here
  for (int l = 0; l + 1 < nl && !g_f32_dict; ++l) {
    const Level& L = s->lv[l];
    if (L.A_rows.dict || (jac && L.A_cols().dict))
      return fail(AMG_HIP_EUNSUPPORTED,
                  "single-precision cycle: level " + std::to_string(l) +
                      " is stored in the dictionary layout (AMG_HIP_LAYOUT_DICT), which has no float form; "
                      "create the solver with `layout` = AMG_HIP_LAYOUT_SELL");
  }
  hipStream_t st = s->stream;
  amg_hip_status r;
  std::vector<F32Level> lv((size_t)nl);
  for (int l = 0; l < nl; ++l) {
    AMG_TRY(ensure_axis_rows(s->lv[l]));  // kind 3: the float transfers are the CSR kernels
    const Level& L = s->lv[l];
    F32Level& Q = lv[(size_t)l];
    const size_t bytes = sizeof(float) * (size_t)L.n;
    HIP_TRY(Q.u.alloc(bytes));
    HIP_TRY(Q.f.alloc(bytes));
    // The coarsest level only takes the direct solve.  With a line smoother it still gets a float matrix,
    // r and factors (it is small), so that amg_hip_f32_line_subsweep runs on every level as
    // amg_hip_level_op does in double: a level of one row is always the coarsest.
    const bool last = l + 1 == nl;
    if (last && (!line || L.A_rows.dict)) continue;
    HIP_TRY(Q.r.alloc(bytes));
    if (line && (r = f32_copy_line_factors(s, L, &Q, st)) != AMG_HIP_OK) return r;
    if ((r = f32_copy_values(L.A_rows, &Q.rows, st)) != AMG_HIP_OK) return r;
    if (last) continue;
    HIP_TRY(Q.tmp.alloc(bytes));
    if (s->opt.smoother == AMG_HIP_SM_CHEBYSHEV) HIP_TRY(Q.d.alloc(bytes));
    if (jac && !L.symmetric)
      if ((r = f32_copy_values(L.A_cols_own, &Q.cols_own, st)) != AMG_HIP_OK) return r;
    if (!(L.linear && s->opt.stencil_transfers) && !L.tensor_stencil) {
      HIP_TRY(Q.pval.alloc(sizeof(float) * (size_t)std::max<int64_t>(L.P_rows.nnz, 1)));
      HIP_TRY(Q.rval.alloc(sizeof(float) * (size_t)std::max<int64_t>(L.R_rows.nnz, 1)));
      HIP_TRY(launch_to_f32(L.P_rows.nnz, L.P_rows.v(), Q.pval.as<float>(), st));
      HIP_TRY(launch_to_f32(L.R_rows.nnz, L.R_rows.v(), Q.rval.as<float>(), st));
    }
  }
  const size_t cb = sizeof(double) * (size_t)s->lv[(size_t)nl - 1].n;
  HIP_TRY(F.cf.alloc(cb));
  HIP_TRY(F.cy.alloc(cb));
  HIP_TRY(F.cx.alloc(cb));
  F.lv = std::move(lv);
  for (int l = 0; l + 1 < nl; ++l) {  // after the move: the vector's storage is final
    F32Level& Q = F.lv[(size_t)l];
    Q.cols = (jac && !s->lv[l].symmetric) ? &Q.cols_own : &Q.rows;
  }
  F.ready = true;
  return AMG_HIP_OK;
}

// one launch of a level matrix in float; bytes: SELL 4 + w per entry and 8 per panel, CSR 8 per
// entry and 4 per row pointer, dictionary the double matrix's stream (layout_of) with 4-byte values in
// the pair table
hipError_t launch_mat_f32(int mode, const F32Mat& M, const float* x, const float* f, float* out, float omega,
                          float* dvec, float alpha, hipStream_t st) {
  const DevMat& A = *M.src;
  if (A.dict) {
    if (A.dict_shift != 0) return hipErrorInvalidValue;  // window blocks: refused before (f32_supported)
    return launch_dict_f32(mode, A.n_rows, A.dict_ref(), M.val.as<float>(), x, f, out, omega, dvec, alpha, st);
  }
  if (A.sell)
    return launch_sell_f32(mode, A.n_rows, A.idx16, A.soff.as<int64_t>(), A.scol.p, M.val.as<float>(), x, f, out,
                           omega, dvec, alpha, st);
  const DevCsr& C = A.csr;
  return launch_csr_f32(mode, C.n_rows, C.rowptr(), C.col(), M.val.as<float>(), x, f, out, omega, dvec, alpha, st);
}
double mat_bytes_f32(const F32Mat& M) {
  const DevMat& A = *M.src;
  if (A.dict)
    return (A.dict_typed ? (double)A.n_rows + 256.0 * 8.0 * (double)A.dict_words
                         : 8.0 * (double)A.dict_words * (double)A.n_rows) +
           8.0 * (double)A.dict_ntab;
  if (A.sell) return (double)A.slots * ((A.idx16 & 1) ? 6.0 : 8.0) + 8.0 * (double)((A.n_rows + 63) / 64);
  return 8.0 * (double)A.csr.nnz + 4.0 * (double)(A.csr.n_rows + 1);
}

// The steps of the float cycle, one member each: enqueue_f32_vcycle strings them together, and
// amg_hip_f32_level_op (a test hook) runs one of them alone -- the same launches either way.
struct F32Steps {
  amg_hip_solver* s;
  StepCtx& X;

  // One sub-sweep of a line smoother in float (launch_line_sweep / launch_alt_subsweep on the float
  // copies): r = f - A u, K-LineSeam on r where direction d is cyclic, u += omega T^-1 r.  LINE_JACOBI:
  // d = 0.  Bytes: the matrix pass; then half of the double solve's (LineOnDev::solve_bytes,
  // AltOnDev::solve_bytes).
  amg_hip_status line_subsweep(int l, int d) {
    const Level& L = s->lv[l];
    F32Level& Q = s->f32.lv[(size_t)l];
    float* u = Q.u.as<float>();
    float* r = Q.r.as<float>();
    const float omega = (float)s->opt.omega;
    STEP_TRY(X, launch_mat_f32(CSR_RESID, Q.rows, u, Q.f.as<float>(), r, 1.0f, nullptr, 0.0f, X.st));
    X.count(mat_bytes_f32(Q.rows) + 12.0 * (double)L.n);  // matrix; u, f in and r out
    if (s->opt.smoother == AMG_HIP_SM_LINE_JACOBI) {
      STEP_TRY(X, launch_line_dir<float>(Q.line.ref(L.line), nullptr, nullptr, 0, r, Q.line.y.as<float>(), u, omega,
                                         X.st));
      X.count(0.5 * L.line.solve_bytes());
      return AMG_HIP_OK;
    }
    const AltOnDev& D = L.alt;
    const SeamRefT<float> S = Q.seam(D, d);
    const LineXRefT<float> LX = Q.xref(D);
    const int k = D.yz_of(d);
    STEP_TRY(X, launch_line_dir(Q.yz[k].ref(D.yz[k]), D.along_x(d) ? &LX : nullptr, D.cyclic(d) ? &S : nullptr, 0, r,
                                Q.yz[k].y.as<float>(), u, omega, X.st));
    X.count(0.5 * D.solve_bytes(d));
    return AMG_HIP_OK;
  }

  // reverse: the way up (AMG_HIP_SM_LINE_ALT runs its directions descending there)
  amg_hip_status smooth(int l, bool reverse) {
    const Level& L = s->lv[l];
    F32Level& Q = s->f32.lv[(size_t)l];
    const double n = (double)L.n;
    const float* f = Q.f.as<float>();
    if (s->opt.smoother == AMG_HIP_SM_LINE_JACOBI || s->opt.smoother == AMG_HIP_SM_LINE_ALT) {
      // enqueue_smooth's order: u is updated in place, so nothing has to come home
      return line_subsweeps(s->opt.smoother_iters, line_dirs(s->opt.smoother, L.alt), reverse,
                            [&](int d) { return line_subsweep(l, d); });
    }
    auto copy_home = [&] {
      STEP_TRY(X, hipMemcpyAsync(Q.u.p, Q.tmp.p, sizeof(float) * (size_t)L.n, hipMemcpyDeviceToDevice, X.st));
      X.count(8.0 * n);
      return AMG_HIP_OK;
    };
    if (s->opt.smoother == AMG_HIP_SM_JACOBI) {
      return ping_pong(s->opt.smoother_iters, Q.u.as<float>(), Q.tmp.as<float>(), [&](int64_t, float* a, float* b) {
        STEP_TRY(X, launch_mat_f32(CSR_JACOBI, *Q.cols, a, f, b, (float)s->opt.omega, nullptr, 0.0f, X.st));
        X.count(mat_bytes_f32(*Q.cols) + 12.0 * n);  // matrix; x, f, out
        return AMG_HIP_OK;
      }, copy_home);
    }
    // the coefficients in double, rounded at the launch
    return cheb_steps(L.cheb_lo, L.cheb_hi, s->opt.smoother_iters, s->opt.cheb_degree, Q.u.as<float>(),
                      Q.tmp.as<float>(), [&](double alpha, double beta, bool first, bool last, float* a, float* b) {
      STEP_TRY(X, launch_mat_f32(cheb_kernel_mode(first, last), Q.rows, a, f, b, (float)beta, Q.d.as<float>(),
                                 (float)alpha, X.st));
      X.count(mat_bytes_f32(Q.rows) + 12.0 * n + (first ? 0.0 : 4.0 * n) + (last ? 0.0 : 4.0 * n));
      return AMG_HIP_OK;
    }, copy_home);
  }

  // r_l = f_l - A_l u_l (:272-274)
  amg_hip_status residual(int l) {
    const Level& L = s->lv[l];
    F32Level& Q = s->f32.lv[(size_t)l];
    STEP_TRY(X, launch_mat_f32(CSR_RESID, Q.rows, Q.u.as<float>(), Q.f.as<float>(), Q.r.as<float>(), 1.0f, nullptr,
                               0.0f, X.st));
    X.count(mat_bytes_f32(Q.rows) + 12.0 * (double)L.n);
    return AMG_HIP_OK;
  }

  // u_{l+1} = 0, f_{l+1} = R_l r_l (:278 + :281-282)
  amg_hip_status restriction(int l) {
    const Level& L = s->lv[l];
    const Level& C = s->lv[l + 1];
    F32Level& Q = s->f32.lv[(size_t)l];
    F32Level& QC = s->f32.lv[(size_t)l + 1];
    if (L.linear && s->opt.stencil_transfers) {
      STEP_TRY(X, launch_linear_restrict_f32(L.n, C.n, Q.r.as<float>(), QC.f.as<float>(), QC.u.as<float>(), X.st));
      X.count(4.0 * (double)L.n + 8.0 * (double)C.n);
    } else if (L.tensor_stencil) {
      STEP_TRY(X, launch_tensor_restrict_f32(L.tdim, L.dims, L.tmask, L.tsides, L.tper, Q.r.as<float>(),
                                             QC.f.as<float>(), QC.u.as<float>(), X.st));
      X.count(4.0 * (double)L.n + 8.0 * (double)C.n);
    } else {
      STEP_TRY(X, launch_zero_f32(C.n, QC.u.as<float>(), X.st));  // as the zero guess: no memset node
      const DevCsr& R = L.R_rows;
      STEP_TRY(X, launch_csr_f32(CSR_SPMV, R.n_rows, R.rowptr(), R.col(), Q.rval.as<float>(), Q.r.as<float>(), nullptr,
                                 QC.f.as<float>(), 1.0f, nullptr, 0.0f, X.st));
      X.count(8.0 * (double)R.nnz + 4.0 * (double)(R.n_rows + 1) + 4.0 * (double)L.n + 8.0 * (double)C.n);
    }
    return AMG_HIP_OK;
  }

  // :287-288 in double: widen f_L, the solver's factor, round the result
  amg_hip_status coarse() {
    F32& F = s->f32;
    const Level& C = s->lv.back();
    F32Level& QC = F.lv.back();
    STEP_TRY(X, launch_to_f64(C.n, QC.f.as<float>(), F.cf.as<double>(), X.st));
    STEP_TRY(X, launch_coarse(s->coarse, F.cf.as<double>(), F.cy.as<double>(), F.cx.as<double>(), X.st));
    STEP_TRY(X, launch_to_f32(C.n, F.cx.as<double>(), QC.u.as<float>(), X.st));
    // the two conversions; the band of L forwards and backwards, D, f, u (enqueue_vcycle_body)
    X.count(24.0 * (double)C.n + 16.0 * (double)C.n * (double)std::max<int64_t>(s->coarse.w, 1) + 24.0 * (double)C.n);
    return AMG_HIP_OK;
  }

  // u_l = u_l + P_l u_{l+1} (:294-296)
  amg_hip_status prolong(int l) {
    const Level& L = s->lv[l];
    const Level& C = s->lv[l + 1];
    F32Level& Q = s->f32.lv[(size_t)l];
    F32Level& QC = s->f32.lv[(size_t)l + 1];
    if (L.linear && s->opt.stencil_transfers) {
      STEP_TRY(X, launch_linear_prolong_add_f32(L.n, C.n, QC.u.as<float>(), Q.u.as<float>(), X.st));
      X.count(4.0 * (double)C.n + 8.0 * (double)L.n);
    } else if (L.tensor_stencil) {
      STEP_TRY(X, launch_tensor_prolong_add_f32(L.tdim, L.dims, L.tmask, L.tsides, L.tper, QC.u.as<float>(),
                                                Q.u.as<float>(), X.st));
      X.count(4.0 * (double)C.n + 8.0 * (double)L.n);
    } else {
      const DevCsr& P = L.P_rows;  // u_h = u_h + P u_H in one launch
      STEP_TRY(X, launch_csr_f32(CSR_SPMV_ADD, P.n_rows, P.rowptr(), P.col(), Q.pval.as<float>(), QC.u.as<float>(),
                                 Q.u.as<float>(), Q.u.as<float>(), 1.0f, nullptr, 0.0f, X.st));
      X.count(8.0 * (double)P.nnz + 4.0 * (double)(P.n_rows + 1) + 4.0 * (double)C.n + 8.0 * (double)L.n);
    }
    return AMG_HIP_OK;
  }
};

// level 0's f holds the right-hand side, its u receives the result
amg_hip_status enqueue_f32_vcycle(amg_hip_solver* s, StepCtx& X) {
  // the zero guess.  A kernel, not hipMemsetAsync: a memset node of the captured graph was seen to fill
  // with stale bytes when the graph is replayed after a device-to-host copy (64 x 48 grid, 12288 bytes)
  STEP_TRY(X, launch_zero_f32(s->lv[0].n, s->f32.lv[0].u.as<float>(), X.st));
  X.count(4.0 * (double)s->lv[0].n);
  return walk_vcycle((int)s->lv.size(), F32Steps{s, X});
}
#undef STEP_TRY

// z = M32^-1 v: round v into level 0's float right-hand side, the cycle (its captured graph, or the
// same enqueue eagerly with use_graph = 0), widen level 0's float solution into z
amg_hip_status f32_apply(amg_hip_solver* s, const double* v, double* z) {
  F32& F = s->f32;
  const int64_t n = s->lv[0].n;
  HIP_TRY(launch_to_f32(n, v, F.lv[0].f.as<float>(), s->stream));
  AMG_TRY(replay_or_enqueue(s->opt.use_graph, F.graph, s->stream, [s] {
    StepCtx X{s->stream};
    return enqueue_f32_vcycle(s, X);
  }));
  HIP_TRY(launch_to_f64(n, F.lv[0].u.as<float>(), z, s->stream));
  return AMG_HIP_OK;
}

}  // namespace

namespace amg_hip {
// for the other translation units of the library (comm.cpp): sets amg_hip_last_error
amg_hip_status fail_status(amg_hip_status st, const std::string& msg) { return fail(st, msg); }
}  // namespace amg_hip

// =============================================================================
extern "C" {

const char* amg_hip_last_error(void) { return g_err.c_str(); }

// `cyclic_lines` sits in the alignment padding that the struct had in front of `stream`: no other field
// moves and the size stays, so callers built against the earlier header pass a valid struct
static_assert(offsetof(amg_hip_options, cyclic_lines) == 68 && offsetof(amg_hip_options, stream) == 72 &&
                  offsetof(amg_hip_options, singular) == 108 && sizeof(amg_hip_options) == 112,
              "amg_hip_options: the layout of the earlier releases must not move");
void amg_hip_default_options(amg_hip_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->smoother = AMG_HIP_SM_SPGS;
  o->smoother_iters = 1;
  o->omega = 1.0;
  o->device = -1;
  o->use_graph = 1;
  o->stencil_transfers = 1;
  o->layout = g_default_layout;
  o->keep_structural_zeros = 0;
  o->no_fusion = 0;
  o->fuse_prolong = 0;
  o->fast_coarse_solve = 0;
  o->stream = nullptr;
  o->window = 0;
  o->cheb_degree = 2;
  o->cheb_lower = 0.3;
  o->cheb_upper = 1.0;
}

void amg_hip_set_index16(int32_t on) { g_index16 = on ? 1 : 0; }
void amg_hip_set_nontemporal(int32_t on) { g_nontemporal = on ? 1 : 0; }
void amg_hip_set_xcd_mapping(int32_t on) { set_xcd_mapping(on); }
void amg_hip_set_row_types(int32_t on) { g_row_types = on ? 1 : 0; }
void amg_hip_set_dict_rows(int32_t rows_per_lane) { set_dict_rows_per_lane(rows_per_lane); }
void amg_hip_set_dict_stencil(int32_t on) { set_dict_stencil(on); }
void amg_hip_set_patch_tile_flags(int32_t on) { g_patch_tile_flags = on ? 1 : 0; }
void amg_hip_set_axis_stencil(int32_t on) { g_axis_stencil = on ? 1 : 0; }
void amg_hip_set_patch_xf(int32_t on) { g_patch_xf = on ? 1 : 0; }
void amg_hip_set_patch_tall(int32_t on) { g_patch_tall = on ? 1 : 0; }
void amg_hip_set_patch_seam(int32_t on) { g_patch_seam = on ? 1 : 0; }
void amg_hip_set_patch_coltype(int32_t on) { g_patch_coltype = on ? 1 : 0; }
void amg_hip_set_band_chain(int32_t on) { g_no_band_chain = on ? 0 : 1; }
void amg_hip_set_tail_fusion(int32_t on) { g_tail_fusion = on ? 1 : 0; }
void amg_hip_set_pair_duo(int32_t on) { g_pair_duo = on ? 1 : 0; }
int32_t amg_hip_pair_duo_partner(const amg_hip_solver* s, int32_t level) {
  if (!s || level < 0 || level >= (int32_t)s->lv.size()) return -1;
  const LegForm up = current_plan(s).lv[(size_t)level].up;
  return up == LEG_DUO_FINE ? level + 1 : (up == LEG_DUO_COARSE ? level - 1 : -1);
}
int32_t amg_hip_duo_windows(int32_t hb_l, int32_t hb_l1, int32_t tile_rows, int32_t* out) {
  return duo_windows_host(hb_l, hb_l1, tile_rows, out);
}
int32_t amg_hip_duo_owned(int32_t tile, int32_t tile_rows, int32_t* out) { return duo_owned_host(tile, tile_rows, out); }
int32_t amg_hip_duo_tile_rows(int32_t hb_l) { return hb_l < 0 ? -1 : duo_tile_rows(hb_l); }
void amg_hip_set_periodic_device_setup(int32_t on) { g_periodic_device_setup = on ? 1 : 0; }
void amg_hip_set_f32_lines(int32_t on) { g_f32_lines = on ? 1 : 0; }
void amg_hip_set_f32_dict(int32_t on) { g_f32_dict = on ? 1 : 0; }
void amg_hip_set_block_lines(int32_t on) { g_block_lines = on ? 1 : 0; }
void amg_hip_set_patch_min_rows(int64_t rows) { g_patch_min_rows = rows < 0 ? INT64_MAX : rows; }

void amg_hip_set_default_layout(int32_t layout) {
  if (layout >= AMG_HIP_LAYOUT_AUTO && layout <= AMG_HIP_LAYOUT_DICT) g_default_layout = layout;
}

int amg_hip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

amg_hip_status amg_hip_create(int64_t n, const int32_t* colptr, const int32_t* rowind,
                              const double* val, const double* b, int32_t n_levels,
                              const amg_hip_options* opts, amg_hip_solver** out) {
  return build_solver(n, colptr, rowind, val, b, n_levels, opts, out);
}

amg_hip_status amg_hip_create_custom(int64_t n, const int32_t* colptr, const int32_t* rowind,
                                     const double* val, const double* b, int32_t n_levels,
                                     const int32_t* const* P_colptr,
                                     const int32_t* const* P_rowind, const double* const* P_val,
                                     const int32_t* const* R_colptr,
                                     const int32_t* const* R_rowind, const double* const* R_val,
                                     const amg_hip_options* opts, amg_hip_solver** out) {
  if (n_levels > 1 && (!P_colptr || !P_rowind || !P_val || !R_colptr || !R_rowind || !R_val))
    return fail(AMG_HIP_EINVAL, "custom transfer operator arrays are null");
  HierarchySpec h;
  h.Pc = P_colptr, h.Pr = P_rowind, h.Pv = P_val;
  h.Rc = R_colptr, h.Rr = R_rowind, h.Rv = R_val;
  return build_solver(n, colptr, rowind, val, b, n_levels, opts, out, h);
}

amg_hip_status amg_hip_create_rs(int64_t n, const int32_t* colptr, const int32_t* rowind,
                                 const double* val, const double* b, int32_t max_levels,
                                 double theta, int64_t min_coarse, const amg_hip_options* opts,
                                 amg_hip_solver** out) {
  if (!(theta >= 0.0 && theta <= 1.0)) return fail(AMG_HIP_EINVAL, "`theta` must be in [0, 1]");
  if (min_coarse < 1) return fail(AMG_HIP_EINVAL, "`min_coarse` must be at least 1");
  HierarchySpec h;
  h.rs_theta = theta;
  h.rs_min_coarse = min_coarse;
  return build_solver(n, colptr, rowind, val, b, max_levels, opts, out, h);
}

static std::string tensor_dims_error(int32_t dim, const int64_t* dims) {
  if (dim != 2 && dim != 3) return "`dim` must be 2 or 3";
  if (!dims) return "`dims` is null";
  if (dims[0] < 1 || dims[1] < 1 || dims[2] < 1) return "every entry of `dims` must be at least 1";
  if (dim == 2 && dims[2] != 1) return "`dims[2]` must be 1 when `dim` is 2";
  if (dims[0] >= ((int64_t)1 << 31) / dims[1] / dims[2]) return "the grid has 2^31 points or more";
  return "";
}

// "" or why a hierarchy of this kind ("full", "semi") cannot be a window solver's
static std::string window_error(const std::string& who, const char* kind) {
  return who + "window solvers (opt.window) coarsen the flat index; a " + kind + "-coarsening hierarchy is not sharded";
}
// "" or that `n` is not the size of the (valid) grid `dims`; figures: with the numbers
static std::string grid_size_error(int64_t n, const int64_t* dims, bool figures) {
  if (n == dims[0] * dims[1] * dims[2]) return "";
  const std::string grid = std::to_string(dims[0]) + " x " + std::to_string(dims[1]) + " x " +
                           std::to_string(dims[2]) + " grid";
  return "`n`" + (figures ? " = " + std::to_string(n) : "") + " is not the " + (figures ? grid : "number of points") +
         " of `dims`";
}
// The grid arguments of a tensor entry point, with its prefix: `dim` and `dims`, `n` against them,
// and no window solver of this kind of hierarchy.  kind null: a query, which has no options and
// words `n` without the figures.
static amg_hip_status tensor_grid_args(const std::string& who, int64_t n, int32_t dim, const int64_t* dims,
                                       int32_t window, const char* kind) {
  std::string e = tensor_dims_error(dim, dims);
  if (e.empty()) e = grid_size_error(n, dims, kind != nullptr);
  if (!e.empty()) return fail(AMG_HIP_EINVAL, who + e);
  if (kind && window) return fail(AMG_HIP_EUNSUPPORTED, window_error(who, kind));
  return AMG_HIP_OK;
}
// the spec of a tensor hierarchy on the grid `dims`
static HierarchySpec tensor_spec(int32_t dim, const int64_t* dims, const SemiRule* semi = nullptr,
                                 int32_t periodic_axes = 0, bool periodic_ctor = false) {
  HierarchySpec h;
  h.dim = dim;
  h.dims = dims;
  h.semi = semi;
  h.periodic = (uint32_t)periodic_axes;
  h.periodic_ctor = periodic_ctor;
  return h;
}

amg_hip_status amg_hip_create_tensor(int64_t n, const int32_t* colptr, const int32_t* rowind,
                                     const double* val, const double* b, int32_t dim,
                                     const int64_t* dims, int32_t n_levels,
                                     const amg_hip_options* opts, amg_hip_solver** out) {
  amg_hip_options o;
  AMG_TRY(out_and_options(opts, out, &o));
  AMG_TRY(tensor_grid_args("amg_hip_create_tensor: ", n, dim, dims, o.window, "full"));
  return build_solver(n, colptr, rowind, val, b, n_levels, &o, out, tensor_spec(dim, dims));
}

// The rule of the semi-coarsening constructors, before any device call: the explicit masks level by
// level on the grids they produce, or the automatic rule's parameters.
static amg_hip_status semi_args(const std::string& who, int32_t dim, const int64_t* dims, int32_t n_levels,
                                const SemiRule& rule) {
  if (n_levels < 1) return fail(AMG_HIP_EINVAL, "`n_levels` must be at least 1");
  if (rule.masks) {
    const std::string e = level_walk_error(who, dim, dims, n_levels, rule.masks, 0, rule.opdep);
    return e.empty() ? AMG_HIP_OK : fail(AMG_HIP_EINVAL, e);
  }
  if (!(rule.theta > 0.0 && rule.theta <= 1.0)) return fail(AMG_HIP_EINVAL, who + "`theta` must be in (0, 1]");
  if (rule.min_coarse < 1) return fail(AMG_HIP_EINVAL, who + "`min_coarse` must be at least 1");
  return AMG_HIP_OK;
}

amg_hip_status amg_hip_create_tensor_semi(int64_t n, const int32_t* colptr, const int32_t* rowind,
                                          const double* val, const double* b, int32_t dim, const int64_t* dims,
                                          int32_t n_levels, const int32_t* axis_masks, double theta,
                                          int64_t min_coarse, const amg_hip_options* opts, amg_hip_solver** out) {
  static const std::string who = "amg_hip_create_tensor_semi: ";
  amg_hip_options o;
  AMG_TRY(out_and_options(opts, out, &o));
  AMG_TRY(tensor_grid_args(who, n, dim, dims, o.window, "semi"));
  const SemiRule rule{axis_masks, theta, min_coarse};
  AMG_TRY(semi_args(who, dim, dims, n_levels, rule));
  return build_solver(n, colptr, rowind, val, b, n_levels, &o, out, tensor_spec(dim, dims, &rule));
}

// Operator-dependent interpolation, one axis per level (host_setup.hpp: axis_opdep_P).  The checks are
// amg_hip_create_tensor_semi's; on top of them every explicit mask names exactly one axis.
amg_hip_status amg_hip_create_tensor_opdep(int64_t n, const int32_t* colptr, const int32_t* rowind,
                                           const double* val, const double* b, int32_t dim, const int64_t* dims,
                                           int32_t n_levels, const int32_t* axis_masks, int64_t min_coarse,
                                           const amg_hip_options* opts, amg_hip_solver** out) {
  static const std::string who = "amg_hip_create_tensor_opdep: ";
  amg_hip_options o;
  AMG_TRY(out_and_options(opts, out, &o));
  AMG_TRY(tensor_grid_args(who, n, dim, dims, o.window, "single-axis"));
  SemiRule rule{axis_masks, 1.0, min_coarse};  // theta: not used; min_coarse: checked and used without masks only
  rule.opdep = true;
  AMG_TRY(semi_args(who, dim, dims, n_levels, rule));
  return build_solver(n, colptr, rowind, val, b, n_levels, &o, out, tensor_spec(dim, dims, &rule));
}

// The checks amg_hip_create_tensor_opdep_periodic adds to amg_hip_create_tensor_opdep's, in
// amg_hip_create_tensor_periodic's order and words: the mask itself, the explicit masks on every
// level's grid (they passed the rule's own checks already), the sides a periodic axis cannot have.
static amg_hip_status opdep_periodic_args(const std::string& who, int32_t dim, const int64_t* dims,
                                          int32_t periodic_axes, int32_t n_levels, const int32_t* axis_masks,
                                          const amg_hip_options& o) {
  const std::string pe = periodic_axes_error(dim, periodic_axes);
  if (!pe.empty()) return fail(AMG_HIP_EINVAL, who + pe);
  if (axis_masks) {
    const std::string le = level_walk_error(who, dim, dims, n_levels, axis_masks, (uint32_t)periodic_axes, true);
    if (!le.empty()) return fail(AMG_HIP_EINVAL, le);
  }
  const std::string se = sides_error(o, dim, (uint32_t)periodic_axes, false);
  if (!se.empty()) return fail(AMG_HIP_EINVAL, se);
  return AMG_HIP_OK;
}

// amg_hip_create_tensor_opdep with periodic axes: its checks under this name, then the periodic ones.
amg_hip_status amg_hip_create_tensor_opdep_periodic(int64_t n, const int32_t* colptr, const int32_t* rowind,
                                                    const double* val, const double* b, int32_t dim,
                                                    const int64_t* dims, int32_t periodic_axes, int32_t n_levels,
                                                    const int32_t* axis_masks, int64_t min_coarse,
                                                    const amg_hip_options* opts, amg_hip_solver** out) {
  static const std::string who = "amg_hip_create_tensor_opdep_periodic: ";
  amg_hip_options o;
  AMG_TRY(out_and_options(opts, out, &o));
  AMG_TRY(tensor_grid_args(who, n, dim, dims, o.window, "single-axis"));
  SemiRule rule{axis_masks, 1.0, min_coarse};
  rule.opdep = true;
  rule.opdep_who = "amg_hip_create_tensor_opdep_periodic: ";
  rule.opdep_periodic = true;
  AMG_TRY(semi_args(who, dim, dims, n_levels, rule));
  AMG_TRY(opdep_periodic_args(who, dim, dims, periodic_axes, n_levels, axis_masks, o));
  return build_solver(n, colptr, rowind, val, b, n_levels, &o, out, tensor_spec(dim, dims, &rule, periodic_axes));
}

amg_hip_status amg_hip_get_axis_weights(const amg_hip_solver* s, int32_t level, double* W) {
  if (!s || !W) return fail(AMG_HIP_EINVAL, "null argument");
  if (level < 0 || level + 1 >= (int)s->lv.size())
    return fail(AMG_HIP_EINVAL, "level out of range (the coarsest level has no transfers)");
  const Level& L = s->lv[level];
  if (L.axis < 0)
    return fail(AMG_HIP_EINVAL, "amg_hip_get_axis_weights: the solver was not made by amg_hip_create_tensor_opdep");  // or _opdep_periodic
  if (L.axis_W.empty() && !s->opt.host_only) HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(L.ensure_axis_weights());
  std::memcpy(W, L.axis_W.data(), sizeof(double) * L.axis_W.size());
  return AMG_HIP_OK;
}

amg_hip_status amg_hip_get_natural_sides(const amg_hip_solver* s, int32_t* mask) {
  if (!s || !mask) return fail(AMG_HIP_EINVAL, "null argument");
  *mask = (!s->lv.empty() && s->lv[0].tdim) ? (int32_t)s->lv[0].tsides : 0;
  return AMG_HIP_OK;
}

amg_hip_status amg_hip_get_periodic_axes(const amg_hip_solver* s, int32_t* mask) {
  if (!s || !mask) return fail(AMG_HIP_EINVAL, "null argument");
  *mask = (!s->lv.empty() && s->lv[0].tdim) ? (int32_t)s->lv[0].tper : 0;
  return AMG_HIP_OK;
}

// The argument checks of the periodic constructors that need no matrix, before any device call:
// those of amg_hip_create_tensor (axis_masks null) or of amg_hip_create_tensor_semi with explicit
// masks, then the periodic mask on every level's grid, then the sides a periodic axis cannot have.
static amg_hip_status periodic_args(const std::string& who, int64_t n, int32_t dim, const int64_t* dims,
                                    int32_t periodic_axes, int32_t n_levels, const int32_t* axis_masks,
                                    const amg_hip_options& o) {
  AMG_TRY(tensor_grid_args(who, n, dim, dims, o.window, axis_masks ? "semi" : "full"));
  const std::string pe = periodic_axes_error(dim, periodic_axes);
  if (!pe.empty()) return fail(AMG_HIP_EINVAL, who + pe);
  if (n_levels < 1) return fail(AMG_HIP_EINVAL, "`n_levels` must be at least 1");
  const std::string le = level_walk_error(who, dim, dims, n_levels, axis_masks, (uint32_t)periodic_axes);
  if (!le.empty()) return fail(AMG_HIP_EINVAL, le);
  const std::string se = sides_error(o, dim, (uint32_t)periodic_axes, true);
  if (!se.empty()) return fail(AMG_HIP_EINVAL, se);
  return AMG_HIP_OK;
}

amg_hip_status amg_hip_create_tensor_periodic(int64_t n, const int32_t* colptr, const int32_t* rowind,
                                              const double* val, const double* b, int32_t dim, const int64_t* dims,
                                              int32_t periodic_axes, int32_t n_levels, const int32_t* axis_masks,
                                              const amg_hip_options* opts, amg_hip_solver** out) {
  amg_hip_options o;
  AMG_TRY(out_and_options(opts, out, &o));
  AMG_TRY(periodic_args("amg_hip_create_tensor_periodic: ", n, dim, dims, periodic_axes, n_levels, axis_masks, o));
  const SemiRule rule{axis_masks};
  return build_solver(n, colptr, rowind, val, b, n_levels, &o, out,
                      tensor_spec(dim, dims, axis_masks ? &rule : nullptr, periodic_axes, true));
}

amg_hip_status amg_hip_get_level_axes(const amg_hip_solver* s, int32_t level, int32_t* axis_mask) {
  if (!s || !axis_mask) return fail(AMG_HIP_EINVAL, "null argument");
  if (level < 0 || level + 1 >= (int)s->lv.size())
    return fail(AMG_HIP_EINVAL, "level out of range (the coarsest level has no transfers)");
  const Level& L = s->lv[level];
  if (!L.tdim || !L.tensor)
    return fail(AMG_HIP_EINVAL, "amg_hip_get_level_axes: the solver was not made by a tensor constructor");
  *axis_mask = (int32_t)L.tmask;
  return AMG_HIP_OK;
}

amg_hip_status amg_hip_tensor_axis_strength(int64_t n, const int32_t* colptr, const int32_t* rowind,
                                            const double* val, int32_t dim, const int64_t* dims, double* w) {
  static const std::string who = "amg_hip_tensor_axis_strength: ";
  if (!colptr || !rowind || !val || !w) return fail(AMG_HIP_EINVAL, "null argument");
  AMG_TRY(tensor_grid_args(who, n, dim, dims, 0, nullptr));
  const Sparse A = from_raw(n, n, colptr, rowind, val);
  const std::string v = validate(A, "A");
  if (!v.empty()) return fail(AMG_HIP_EINVAL, v);
  tensor_axis_strength(A, dim, dims, w);
  return AMG_HIP_OK;
}

amg_hip_status amg_hip_get_level_dims(const amg_hip_solver* s, int32_t level, int64_t* dims) {
  if (!s || !dims) return fail(AMG_HIP_EINVAL, "null argument");
  if (level < 0 || level >= (int)s->lv.size()) return fail(AMG_HIP_EINVAL, "level out of range");
  const Level& L = s->lv[level];
  if (!L.tdim)
    return fail(AMG_HIP_EINVAL, "amg_hip_get_level_dims: the solver was not made by amg_hip_create_tensor");
  for (int a = 0; a < 3; ++a) dims[a] = L.dims[a];
  return AMG_HIP_OK;
}

amg_hip_status amg_hip_level_transfer_kind(const amg_hip_solver* s, int32_t level, int32_t* kind) {
  if (!s || !kind) return fail(AMG_HIP_EINVAL, "null argument");
  if (level < 0 || level + 1 >= (int)s->lv.size())
    return fail(AMG_HIP_EINVAL, "level out of range (the coarsest level has no transfers)");
  const Level& L = s->lv[level];
  *kind = L.axis_stencil ? 3 : (L.tensor_stencil ? 2 : ((L.linear && s->opt.stencil_transfers) ? 1 : 0));
  return AMG_HIP_OK;
}

amg_hip_status amg_hip_create_poisson(int32_t dim, int64_t n, int32_t n_levels,
                                      const amg_hip_options* opts, amg_hip_solver** out) {
  amg_hip_options o;
  AMG_TRY(out_and_options(opts, out, &o));
  if ((dim != 2 && dim != 3) || n < 1) return fail(AMG_HIP_EINVAL, "dim must be 2 or 3 and n >= 1");
  {
    const std::string e = sides_error(o, 0);
    if (!e.empty()) return fail(AMG_HIP_EINVAL, "amg_hip_create_poisson: " + e);
  }
  bool unsupported = true;
  amg_hip_status r = build_poisson_device(dim, n, n_levels, o, out, &unsupported);
  if (r != AMG_HIP_OK || !unsupported) return r;
  // options that need host structures: generate on the host and take the general constructor
  Sparse A = laplacian(dim, n);
  std::vector<double> b((size_t)A.n_outer);
  rhs_threads(dim, n, b.data(), host_threads());
  return build_solver(A.n_outer, A.ptr.data(), A.idx.data(), A.val.data(), b.data(), n_levels, &o, out);
}

amg_hip_status amg_hip_create_poisson_tensor(int32_t dim, int64_t n, int32_t n_levels,
                                             const amg_hip_options* opts, amg_hip_solver** out) {
  static const std::string who = "amg_hip_create_poisson_tensor: ";
  amg_hip_options o;
  AMG_TRY(out_and_options(opts, out, &o));
  if (dim != 2 && dim != 3) return fail(AMG_HIP_EINVAL, "amg_hip_create_poisson_tensor: `dim` must be 2 or 3");
  if (n < 2) return fail(AMG_HIP_EINVAL, "amg_hip_create_poisson_tensor: `n` must be at least 2");
  if (n >= ((int64_t)1 << 31) / n / (dim == 3 ? n : 1))
    return fail(AMG_HIP_EINVAL, "amg_hip_create_poisson_tensor: the grid has 2^31 points or more");
  if (n_levels < 1) return fail(AMG_HIP_EINVAL, "`n_levels` must be at least 1");
  {  // the model problem is Dirichlet on every side
    const std::string e = sides_error(o, 0);
    if (!e.empty()) return fail(AMG_HIP_EINVAL, who + e);
  }
  if (o.window) return fail(AMG_HIP_EUNSUPPORTED, window_error(who, "full"));
  const int64_t dims[3] = {n, n, dim == 3 ? n : 1};
  {  // the levels the rule allows, before the device is touched
    const std::string e = level_walk_error(who, dim, dims, n_levels, nullptr, 0);
    if (!e.empty()) return fail(AMG_HIP_EINVAL, e);
  }
  if (o.smoother == AMG_HIP_SM_CHEBYSHEV) {  // ahead of the other options: the order of this entry point
    const std::string e = cheb_options_error(o.cheb_degree, o.cheb_lower, o.cheb_upper);
    if (!e.empty()) return fail(AMG_HIP_EINVAL, e);
  }
  bool unsupported = true;
  amg_hip_status r = build_poisson_device(dim, n, n_levels, o, out, &unsupported, 0, -1, true);
  if (r != AMG_HIP_OK || !unsupported) return r;
  // options that need host structures: generate on the host and take the host constructor
  Sparse A = laplacian(dim, n);
  std::vector<double> b((size_t)A.n_outer);
  rhs_threads(dim, n, b.data(), host_threads());
  return build_solver(A.n_outer, A.ptr.data(), A.idx.data(), A.val.data(), b.data(), n_levels, &o, out,
                      tensor_spec(dim, dims));
}

// Front end of amg_hip_create_tensor_dev: the caller's device arrays are copied on the solver's
// stream and checked by K-CsrCheck; then the level loop, unless the options need host structures.
// *unsupported = true on return with AMG_HIP_OK: the (checked) matrix takes the host constructor.
static amg_hip_status build_tensor_user_device(const std::string& who, int64_t n, const int32_t* rowptr,
                                               const int32_t* col, const double* val, const double* b,
                                               int32_t n_levels, const HierarchySpec& h, const amg_hip_options& o,
                                               amg_hip_solver** out, bool* unsupported) {
  *unsupported = true;
  std::unique_ptr<amg_hip_solver> s;
  AMG_TRY(device_setup_begin(o, &s));
  SetupLap lap;
  DevCsr cur;
  DevMem rhs, bad;
  const hipStream_t st = s->stream;
  HIP_TRY(cur.ptr.alloc(sizeof(int32_t) * (n + 1)));
  HIP_TRY(hipMemcpyAsync(cur.ptr.p, rowptr, sizeof(int32_t) * (n + 1), hipMemcpyDeviceToDevice, st));
  int32_t nnz32 = -1;
  HIP_TRY(hipMemcpyAsync(&nnz32, cur.ptr.as<int32_t>() + n, sizeof(int32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (nnz32 < 0 || nnz32 == INT32_MAX)
    return fail(AMG_HIP_EINVAL, who + "`rowptr[n]` = " + std::to_string(nnz32) +
                                    " is not a number of entries (row " + std::to_string(n - 1) + ")");
  const int64_t nnz = nnz32;
  HIP_TRY(cur.idx.alloc(sizeof(int32_t) * std::max<int64_t>(nnz, 1)));
  HIP_TRY(cur.val.alloc(sizeof(double) * std::max<int64_t>(nnz, 1)));
  HIP_TRY(rhs.alloc(sizeof(double) * n));
  HIP_TRY(bad.alloc(sizeof(int32_t)));
  const int32_t none = INT32_MAX;
  int32_t first_bad = none;
  HIP_TRY(hipMemcpyAsync(bad.p, &none, sizeof(int32_t), hipMemcpyHostToDevice, st));
  if (nnz > 0) HIP_TRY(hipMemcpyAsync(cur.idx.p, col, sizeof(int32_t) * nnz, hipMemcpyDeviceToDevice, st));
  HIP_TRY(launch_csr_check(n, nnz, cur.rowptr(), cur.col(), bad.as<int32_t>(), st));
  HIP_TRY(hipMemcpyAsync(&first_bad, bad.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
  if (nnz > 0) HIP_TRY(hipMemcpyAsync(cur.val.p, val, sizeof(double) * nnz, hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipMemcpyAsync(rhs.p, b, sizeof(double) * n, hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (first_bad != none)
    return fail(AMG_HIP_EINVAL, who + "row " + std::to_string(first_bad) +
                                    " of the CSR arrays is malformed (`rowptr` must start at 0 and never decrease; "
                                    "the columns of a row must lie in [0, n) and ascend strictly)");
  cur.n_rows = cur.n_cols = n;
  cur.nnz = nnz;
  lap("copy + check");
  const bool on_device = (o.smoother == AMG_HIP_SM_JACOBI || o.smoother == AMG_HIP_SM_CHEBYSHEV ||
                          o.smoother == AMG_HIP_SM_LINE_JACOBI || o.smoother == AMG_HIP_SM_LINE_ALT) &&
                         !o.host_only && !o.host_galerkin && o.stencil_transfers && !o.fuse_prolong && n_levels >= 2 &&
                         n < ((int64_t)1 << 28);
  if (!on_device) return AMG_HIP_OK;
  auto put_rhs = [&](Level& L0) -> amg_hip_status {
    HIP_TRY(hipMemcpy(L0.f.p, rhs.p, sizeof(double) * n, hipMemcpyDeviceToDevice));
    HIP_TRY(hipMemcpy(L0.r.p, rhs.p, sizeof(double) * n, hipMemcpyDeviceToDevice));  // b - A*0
    return AMG_HIP_OK;
  };
  const amg_hip_status r = device_level_loop(s.get(), cur, h, true, n_levels, lap, put_rhs, unsupported);
  if (r != AMG_HIP_OK || *unsupported) return r;
  *out = s.release();
  return AMG_HIP_OK;
}

// amg_hip_create_tensor_dev, amg_hip_create_tensor_semi_dev (rule: what the caller asks) and
// amg_hip_create_tensor_periodic_dev (h.periodic_ctor; rule: its explicit masks, or null).  With
// amg_hip_set_periodic_device_setup(1) the periodic level loop runs on the device with the mask
// (K-TensorGalerkin's PER form); with the default 0 its hierarchy is built on the host (the checked
// arrays take the host constructor) and the level loop on the device is never entered.  The same
// switch governs amg_hip_create_tensor_opdep_periodic_dev (rule->opdep_periodic): on, its levels take
// the PER forms of K-AxisWeights and K-AxisGalerkin, with amg_hip_create_tensor_opdep_dev's fallbacks.
static amg_hip_status create_tensor_dev(const std::string& who, int64_t n, const int32_t* rowptr_dev,
                                        const int32_t* col_dev, const double* val_dev, const double* b_dev,
                                        int32_t n_levels, HierarchySpec h, const SemiRule* rule,
                                        const amg_hip_options* opts, amg_hip_solver** out) {
  amg_hip_options o;
  AMG_TRY(out_and_options(opts, out, &o));
  if (!rowptr_dev || !col_dev || !val_dev || !b_dev) return fail(AMG_HIP_EINVAL, "null input array");
  h.semi = rule;
  if (h.periodic_ctor) {  // grid, masks, levels and sides: the host constructor's one check
    AMG_TRY(periodic_args(who, n, h.dim, h.dims, (int32_t)h.periodic, n_levels, rule ? rule->masks : nullptr, o));
  } else {
    AMG_TRY(tensor_grid_args(who, n, h.dim, h.dims, o.window, rule ? (rule->opdep ? "single-axis" : "semi") : "full"));
    if (n_levels < 1) return fail(AMG_HIP_EINVAL, "`n_levels` must be at least 1");
    if (rule) {
      AMG_TRY(semi_args(who, h.dim, h.dims, n_levels, *rule));
      if (rule->opdep_periodic)
        AMG_TRY(opdep_periodic_args(who, h.dim, h.dims, (int32_t)h.periodic, n_levels, rule->masks, o));
    } else {  // the levels the rule allows
      const std::string e = level_walk_error(who, h.dim, h.dims, n_levels, nullptr, 0);
      if (!e.empty()) return fail(AMG_HIP_EINVAL, e);
    }
  }
  AMG_TRY(smoother_options_error(o, h.dim, n_levels, h.periodic, h.periodic_ctor));
  bool unsupported = true;
  amg_hip_options od = o;
  if (h.periodic_ctor && !g_periodic_device_setup) od.host_galerkin = 1;  // copy + check only
  if (rule && rule->opdep && !g_axis_stencil) od.host_galerkin = 1;       // transfer kind 0 needs CSR(P), CSR(R): host
  if (rule && rule->opdep_periodic && !g_periodic_device_setup) od.host_galerkin = 1;  // copy + check only
  amg_hip_status r = build_tensor_user_device(who, n, rowptr_dev, col_dev, val_dev, b_dev, n_levels, h, od, out,
                                              &unsupported);
  if (r != AMG_HIP_OK || !unsupported) return r;
  // options that need host structures (or a product the kernels refused): the checked arrays are
  // downloaded, transposed on the host and given to the host constructor
  Sparse H;  // CSR(A)
  std::vector<double> b((size_t)n);
  {
    int dev_before = 0;
    HIP_TRY(hipGetDevice(&dev_before));
    if (o.device >= 0) HIP_TRY(hipSetDevice(o.device));
    Scoped own;
    hipStream_t st = (hipStream_t)o.stream;
    if (!st) {
      HIP_TRY(hipStreamCreateWithFlags(&own.st, hipStreamNonBlocking));
      st = own.st;
    }
    HIP_TRY(hipMemcpyAsync(b.data(), b_dev, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    HIP_TRY(download_csr(n, rowptr_dev, col_dev, val_dev, st, &H));
    if (o.device >= 0) HIP_TRY(hipSetDevice(dev_before));
  }
  const Sparse A = transpose(H);  // CSC(A)
  return build_solver(n, A.ptr.data(), A.idx.data(), A.val.data(), b.data(), n_levels, &o, out, h);
}

amg_hip_status amg_hip_create_tensor_dev(int64_t n, const int32_t* rowptr_dev, const int32_t* col_dev,
                                         const double* val_dev, const double* b_dev, int32_t dim,
                                         const int64_t* dims, int32_t n_levels, const amg_hip_options* opts,
                                         amg_hip_solver** out) {
  return create_tensor_dev("amg_hip_create_tensor_dev: ", n, rowptr_dev, col_dev, val_dev, b_dev, n_levels,
                           tensor_spec(dim, dims), nullptr, opts, out);
}

amg_hip_status amg_hip_create_tensor_semi_dev(int64_t n, const int32_t* rowptr_dev, const int32_t* col_dev,
                                              const double* val_dev, const double* b_dev, int32_t dim,
                                              const int64_t* dims, int32_t n_levels, const int32_t* axis_masks,
                                              double theta, int64_t min_coarse, const amg_hip_options* opts,
                                              amg_hip_solver** out) {
  const SemiRule rule{axis_masks, theta, min_coarse};
  return create_tensor_dev("amg_hip_create_tensor_semi_dev: ", n, rowptr_dev, col_dev, val_dev, b_dev, n_levels,
                           tensor_spec(dim, dims), &rule, opts, out);
}

amg_hip_status amg_hip_create_tensor_opdep_dev(int64_t n, const int32_t* rowptr_dev, const int32_t* col_dev,
                                               const double* val_dev, const double* b_dev, int32_t dim,
                                               const int64_t* dims, int32_t n_levels, const int32_t* axis_masks,
                                               int64_t min_coarse, const amg_hip_options* opts, amg_hip_solver** out) {
  SemiRule rule{axis_masks, 1.0, min_coarse};  // as amg_hip_create_tensor_opdep
  rule.opdep = true;
  rule.opdep_who = "amg_hip_create_tensor_opdep_dev: ";
  return create_tensor_dev(rule.opdep_who, n, rowptr_dev, col_dev, val_dev, b_dev, n_levels, tensor_spec(dim, dims), &rule,
                           opts, out);
}

amg_hip_status amg_hip_create_tensor_opdep_periodic_dev(int64_t n, const int32_t* rowptr_dev, const int32_t* col_dev,
                                                        const double* val_dev, const double* b_dev, int32_t dim,
                                                        const int64_t* dims, int32_t periodic_axes, int32_t n_levels,
                                                        const int32_t* axis_masks, int64_t min_coarse,
                                                        const amg_hip_options* opts, amg_hip_solver** out) {
  SemiRule rule{axis_masks, 1.0, min_coarse};  // as amg_hip_create_tensor_opdep_periodic
  rule.opdep = true;
  rule.opdep_who = "amg_hip_create_tensor_opdep_periodic_dev: ";
  rule.opdep_periodic = true;
  return create_tensor_dev(rule.opdep_who, n, rowptr_dev, col_dev, val_dev, b_dev, n_levels,
                           tensor_spec(dim, dims, nullptr, periodic_axes), &rule, opts, out);
}

amg_hip_status amg_hip_create_tensor_periodic_dev(int64_t n, const int32_t* rowptr_dev, const int32_t* col_dev,
                                                  const double* val_dev, const double* b_dev, int32_t dim,
                                                  const int64_t* dims, int32_t periodic_axes, int32_t n_levels,
                                                  const int32_t* axis_masks, const amg_hip_options* opts,
                                                  amg_hip_solver** out) {
  const SemiRule rule{axis_masks};
  return create_tensor_dev("amg_hip_create_tensor_periodic_dev: ", n, rowptr_dev, col_dev, val_dev, b_dev, n_levels,
                           tensor_spec(dim, dims, nullptr, periodic_axes, true), axis_masks ? &rule : nullptr, opts,
                           out);
}

amg_hip_status amg_hip_setup_on_device(const amg_hip_solver* s, int32_t* on) {
  if (!s || !on) return fail(AMG_HIP_EINVAL, "null argument");
  *on = s->device_setup ? 1 : 0;
  return AMG_HIP_OK;
}

amg_hip_status amg_hip_create_poisson_window(int32_t dim, int64_t n, int64_t unit_begin, int64_t unit_end,
                                             int32_t n_levels, const amg_hip_options* opts,
                                             amg_hip_solver** out) {
  amg_hip_options o;
  AMG_TRY(out_and_options(opts, out, &o));
  if ((dim != 2 && dim != 3) || n < 1) return fail(AMG_HIP_EINVAL, "dim must be 2 or 3 and n >= 1");
  if (unit_begin < 0 || unit_end > n || unit_end - unit_begin < 1)
    return fail(AMG_HIP_EINVAL, "window units must satisfy 0 <= unit_begin < unit_end <= n");
  const int64_t unit_rows = dim == 3 ? n * n : n;
  if ((unit_begin * unit_rows) & 1)
    return fail(AMG_HIP_EINVAL, "a window must begin at an even flat index (coarse dof j <-> fine dof 2j+1, multigrid.hpp:127-130)");
  if (n_levels < 2) return fail(AMG_HIP_EINVAL, "a window solver needs at least one distributed level (n_levels >= 2)");
  if (o.smoother == AMG_HIP_SM_LINE_ALT) return fail(AMG_HIP_EINVAL, ALT_NEEDS_GRID);
  {
    const std::string e = sides_error(o, 0);
    if (!e.empty()) return fail(AMG_HIP_EINVAL, "amg_hip_create_poisson_window: " + e);
  }
  if (o.smoother == AMG_HIP_SM_CHEBYSHEV)
    return fail(AMG_HIP_EUNSUPPORTED, "amg_hip_create_poisson_window: the Chebyshev smoother is not sharded");
  if (o.smoother == AMG_HIP_SM_LINE_JACOBI)
    return fail(AMG_HIP_EUNSUPPORTED, "amg_hip_create_poisson_window: the line smoother is not sharded");
  o.window = 1;
  bool unsupported = true;
  amg_hip_status r = build_poisson_device(dim, n, n_levels, o, out, &unsupported, unit_begin, unit_end);
  if (r != AMG_HIP_OK || !unsupported) return r;
  // options that need host structures (multicolouring, ...): generate the window on the host
  Sparse A = laplacian(dim, n, unit_end - unit_begin);
  std::vector<double> b((size_t)A.n_outer);
  rhs_threads(dim, n, b.data(), host_threads(), unit_begin * unit_rows, unit_end * unit_rows);
  return build_solver(A.n_outer, A.ptr.data(), A.idx.data(), A.val.data(), b.data(), n_levels, &o, out);
}

void amg_hip_destroy(amg_hip_solver* s) {
  if (!s) return;
  if (!s->opt.host_only) {
    (void)hipSetDevice(s->device);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
  }
  delete s;
}

amg_hip_status amg_hip_vcycles(amg_hip_solver* s, int32_t n) {
  if (!s) return fail(AMG_HIP_EINVAL, "null solver");
  amg_hip_status r = set_device(s);
  if (r != AMG_HIP_OK) return r;
  if (n >= 2 && current_plan(s).seam) {
    // head, n - 1 seam cycles, finish.  The handed-over level-0 vector alternates between tmp and r;
    // the head starts on the buffer that makes the last seam cycle write tmp, where a stand-alone
    // cycle leaves that vector, so the finish is the cycle's own last launch.
    int src = (n - 1) & 1;
    if ((r = run_seam(s, SEAM_HEAD, src)) != AMG_HIP_OK) return r;
    for (int i = 1; i < n; ++i, src ^= 1)
      if ((r = run_seam(s, SEAM_CYCLE, src)) != AMG_HIP_OK) return r;
    return run_seam(s, SEAM_FINISH, 0);
  }
  return replay_or_enqueue(s->opt.use_graph, s->graph, s->stream, [s] { return enqueue_vcycle(s); }, n);
}
amg_hip_status amg_hip_vcycle(amg_hip_solver* s) { return amg_hip_vcycles(s, 1); }

// ---- slab sharding (struct Slab) ---------------------------------------------
namespace {
// a bigger allocation with the same leading contents
amg_hip_status grow(DevMem& m, size_t bytes, hipStream_t st) {
  if (m.bytes >= bytes) return AMG_HIP_OK;
  DevMem big;
  HIP_TRY(big.alloc(bytes));
  HIP_TRY(hipMemsetAsync(big.p, 0, bytes, st));
  if (m.bytes) HIP_TRY(hipMemcpyAsync(big.p, m.p, m.bytes, hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));
  m = std::move(big);
  return AMG_HIP_OK;
}
}  // namespace

amg_hip_status amg_hip_slab_plan(int64_t lines, int32_t rank, int32_t world, int32_t levels,
                                 amg_hip_slab_info* out) {
  if (!out || lines < 1 || world < 1 || rank < 0 || rank >= world || levels < 1 ||
      levels > AMG_HIP_SLAB_MAX_LEVELS)
    return fail(AMG_HIP_EINVAL, "amg_hip_slab_plan: bad argument");
  const int k = levels;
  std::memset(out, 0, sizeof(*out));
  const int64_t chunk = (lines + world - 1) / world;
  const int64_t line0 = std::min<int64_t>(lines, chunk * rank);
  const int64_t line1 = std::min<int64_t>(lines, chunk * (rank + 1));
  // Lines beyond the owned block on which each leg's INPUT has to be valid.  A Jacobi sweep or
  // a residual makes one line plus one entry (the corner couplings of the 9-point coarse
  // operators) at either end stale; the restriction and the prolongation reach two / one
  // entries across a line end.  Counted in whole lines:
  //   up-leg of level l (prolongation + two sweeps) has to leave u_l valid 3 l lines out (what
  //   level l-1 loads: two sweeps' worth plus the neighbouring coarse entry), so the smoothed
  //   u_l the down-leg left must be valid 3 l + 2 lines and 2 entries out: 3 l + 3 lines;
  //   down-leg of level l: input valid I_l lines out gives f_{l+1} valid I_l - sweeps - 2 lines
  //   out (sweeps, residual, and the restriction's entries: less than a line), where sweeps = 2
  //   on level 0 and 1 below it (the first sweep of a coarser level is done by the finer
  //   level's kernel); the gathered level needs f only on the owned lines.
  std::vector<int64_t> need(k + 1, 0);
  for (int l = k - 1; l >= 0; --l) {
    const int sw = l == 0 ? 2 : 1;
    const int64_t own = 3 * l + 3 + sw;
    const int64_t feed = (l + 1 < k ? need[l + 1] : 0) + 2 + sw;
    need[l] = std::max(own, feed);
  }
  const int64_t last = lines - chunk * (world - 1);
  if (world > 1 && (last < need[0] || chunk < need[0]))
    return fail(AMG_HIP_EUNSUPPORTED, "amg_hip_slab_plan: fewer grid lines per rank than the halo depth");
  auto lo = [&](int64_t h) { return world == 1 ? 0 : std::max<int64_t>(0, line0 - h); };
  auto hi = [&](int64_t h) { return world == 1 ? lines : std::min<int64_t>(lines, line1 + h); };
  for (int l = 0; l < k; ++l) {
    out->down_lo[l] = lo(need[l]);
    out->down_hi[l] = hi(need[l]);
    out->up_lo[l] = lo(3 * l);
    out->up_hi[l] = hi(3 * l);
  }
  out->levels = k;
  out->halo_lines = (int32_t)need[0];
  out->lines = lines;
  out->chunk_lines = chunk;
  out->line_begin = line0;
  out->line_end = line1;
  return AMG_HIP_OK;
}

amg_hip_status amg_hip_slab_setup(amg_hip_solver* s, int32_t rank, int32_t world,
                                  int32_t max_levels, amg_hip_slab_info* info) {
  if (!s || !info || world < 1 || rank < 0 || rank >= world)
    return fail(AMG_HIP_EINVAL, "amg_hip_slab_setup: bad argument");
  if (s->opt.window) return fail(AMG_HIP_EINVAL, "amg_hip_slab_setup: a window solver is cut already (amg_hip_window_setup)");
  if (s->opt.smoother == AMG_HIP_SM_CHEBYSHEV)
    return fail(AMG_HIP_EUNSUPPORTED, "amg_hip_slab_setup: the Chebyshev smoother is not sharded");
  if (s->opt.smoother == AMG_HIP_SM_LINE_JACOBI || s->opt.smoother == AMG_HIP_SM_LINE_ALT)
    return fail(AMG_HIP_EUNSUPPORTED, "amg_hip_slab_setup: the line smoother is not sharded");
  amg_hip_status r = set_device(s);
  if (r != AMG_HIP_OK) return r;
  int k = 0;
  {
    const CyclePlan P = current_plan(s);
    while (k < (int)P.lv.size() && P.lv[(size_t)k].down == LEG_PATCH) ++k;
  }
  if (max_levels >= 0 && k > max_levels) k = max_levels;
  if (k > AMG_HIP_SLAB_MAX_LEVELS) k = AMG_HIP_SLAB_MAX_LEVELS;
  if (k < 1)
    return fail(AMG_HIP_EUNSUPPORTED,
                "amg_hip_slab_setup: no K-Patch level (needs the 2+2 true-Jacobi cycle on a "
                "dictionary-coded 2-D hierarchy of at least patch_min_rows rows)");
  HIP_TRY(hipStreamSynchronize(s->stream));
  Slab& sb = s->slab;
  sb.reset_graphs();
  s->plan_kept = false;
  sb.levels = 0;  // configured again only when everything below succeeds
  const Level& L0 = s->lv[0];
  const int64_t m0 = L0.A_rows.patch_m;
  sb.lines = (L0.n + m0 - 1) / m0;
  for (int l = 0; l <= k; ++l) {  // the lines of the slab levels coincide (x-only coarsening)
    const Level& L = s->lv[l];
    const int64_t m = l < k ? L.A_rows.patch_m : s->lv[k - 1].A_rows.patch_m / 2;
    if (m != (m0 >> l) || (L.n + m - 1) / m != sb.lines)
      return fail(AMG_HIP_EUNSUPPORTED, "amg_hip_slab_setup: level lines do not coincide");
  }
  amg_hip_slab_info pl;
  if ((r = amg_hip_slab_plan(sb.lines, rank, world, k, &pl)) != AMG_HIP_OK) return r;
  sb.rank = rank;
  sb.world = world;
  sb.chunk = pl.chunk_lines;
  sb.line0 = pl.line_begin;
  sb.line1 = pl.line_end;
  sb.halo = pl.halo_lines;
  sb.down_lo.assign(pl.down_lo, pl.down_lo + k);
  sb.down_hi.assign(pl.down_hi, pl.down_hi + k);
  sb.up_lo.assign(pl.up_lo, pl.up_lo + k);
  sb.up_hi.assign(pl.up_hi, pl.up_hi + k);
  sb.levels = k;
  // in-place all-gathers need room for world equal blocks
  Level& G = s->lv[k];
  const int64_t mk = m0 >> k;
  if ((r = grow(G.f, sizeof(double) * (size_t)(sb.chunk * world * mk), s->stream)) != AMG_HIP_OK ||
      (r = grow(s->lv[0].u, sizeof(double) * (size_t)(sb.chunk * world * m0), s->stream)) != AMG_HIP_OK) {
    sb.levels = 0;  // not configured: amg_hip_slab_run refuses
    return r;
  }
  for (CycleGraph& g : s->seam_graph) g.reset();
  s->graph.reset();  // the whole-cycle graph holds the old pointers
  *info = pl;
  info->pitch0 = m0;
  info->gather_pitch = mk;
  info->gather_rows = G.n;
  info->u0 = s->lv[0].u.as<double>();
  info->f_gather = G.f.as<double>();
  return AMG_HIP_OK;
}

amg_hip_status amg_hip_slab_run(amg_hip_solver* s, int32_t part) {
  if (!s || part < CYCLE_SLAB_DOWN || part > CYCLE_SLAB_UP)
    return fail(AMG_HIP_EINVAL, "amg_hip_slab_run: part is 1 (down-legs), 2 (replicated rest) or 3 (up-legs)");
  Slab& sb = s->slab;
  if (sb.levels < 1) return fail(AMG_HIP_EINVAL, "amg_hip_slab_run: amg_hip_slab_setup has not succeeded");
  amg_hip_status r = set_device(s);
  if (r != AMG_HIP_OK) return r;
  return replay_or_enqueue(s->opt.use_graph, sb.graph[part - 1], s->stream,
                           [s, part] { return enqueue_vcycle(s, part); });
}

amg_hip_status amg_hip_window_setup(amg_hip_solver* s, const int64_t* down_lo, const int64_t* down_hi,
                                    const int64_t* up_lo, const int64_t* up_hi) {
  if (!s) return fail(AMG_HIP_EINVAL, "null solver");
  if (!s->opt.window) return fail(AMG_HIP_EINVAL, "amg_hip_window_setup: not a window solver (opt.window)");
  if ((down_lo || down_hi || up_lo || up_hi) && !(down_lo && down_hi && up_lo && up_hi))
    return fail(AMG_HIP_EINVAL, "amg_hip_window_setup: give all four range arrays or none");
  amg_hip_status r = set_device(s);
  if (r != AMG_HIP_OK) return r;
  HIP_TRY(hipStreamSynchronize(s->stream));
  const int k = (int)s->lv.size() - 1;
  Slab& sb = s->slab;
  sb.reset_graphs();
  s->plan_kept = false;
  sb.levels = k;
  sb.rank = 0;
  sb.world = 1;
  sb.down_lo.assign(k, 0);
  sb.down_hi.assign(k, -1);  // -1: every line
  sb.up_lo.assign(k, 0);
  sb.up_hi.assign(k, -1);
  if (down_lo)
    for (int l = 0; l < k; ++l) {
      if (down_lo[l] < 0 || up_lo[l] < 0 || down_hi[l] < down_lo[l] || up_hi[l] < up_lo[l])
        return fail(AMG_HIP_EINVAL, "amg_hip_window_setup: bad line range");
      sb.down_lo[l] = down_lo[l];
      sb.down_hi[l] = down_hi[l];
      sb.up_lo[l] = up_lo[l];
      sb.up_hi[l] = up_hi[l];
    }
  return AMG_HIP_OK;
}

amg_hip_status amg_hip_window_run(amg_hip_solver* s, int32_t part) {
  if (!s || (part != CYCLE_SLAB_DOWN && part != CYCLE_SLAB_UP))
    return fail(AMG_HIP_EINVAL, "amg_hip_window_run: part is 1 (down-legs) or 3 (up-legs)");
  if (!s->opt.window) return fail(AMG_HIP_EINVAL, "amg_hip_window_run: not a window solver (opt.window)");
  if (s->slab.levels < 1) {
    amg_hip_status r = amg_hip_window_setup(s, nullptr, nullptr, nullptr, nullptr);
    if (r != AMG_HIP_OK) return r;
  }
  return amg_hip_slab_run(s, part);
}

#ifdef AMG_PATCH_STAMPS
amg_hip_status amg_hip_debug_patch_stamps(void* dev_ptr) {  // diagnostic build only (tools/patch_stamps.py)
  HIP_TRY(debug_set_patch_stamps((unsigned long long*)dev_ptr));
  return AMG_HIP_OK;
}
amg_hip_status amg_hip_debug_patch_stamps_rows(int32_t rows) {  // 0: every down-leg stamps; else the level of `rows` rows
  HIP_TRY(debug_set_patch_stamps_rows((int)rows));
  return AMG_HIP_OK;
}
#endif

amg_hip_status amg_hip_get_stream(amg_hip_solver* s, void** stream) {
  if (!s || !stream) return fail(AMG_HIP_EINVAL, "bad argument");
  if (s->opt.host_only) return fail(AMG_HIP_EINVAL, "solver was created with host_only = 1: no device state");
  *stream = (void*)s->stream;
  return AMG_HIP_OK;
}

// Where a level's vector lives, for every accessor and the level operations alike: the solution (which
// == 0) where the plan says it rests -- a coarse K-Patch level and the finer level of a K-Duo pair
// leave it in their second buffer -- f and r in their own.
static DevMem* level_vec(amg_hip_solver* s, int32_t level, int32_t which) {
  if (!s || level < 0 || level >= (int32_t)s->lv.size()) return nullptr;
  Level& L = s->lv[level];
  if (which == 0) return current_plan(s).lv[(size_t)level].rests_tmp ? &L.tmp : &L.u;
  return which == 1 ? &L.f : (which == 2 ? &L.r : nullptr);
}
amg_hip_status amg_hip_vec_dev_ptr(amg_hip_solver* s, int32_t level, int32_t which, void** ptr, int64_t* n) {
  if (!s || !ptr || level < 0 || level >= (int32_t)s->lv.size() || which < 0 || which > 2)
    return fail(AMG_HIP_EINVAL, "bad argument");
  if (s->opt.host_only) return fail(AMG_HIP_EINVAL, "solver was created with host_only = 1: no device state");
  Level& L = s->lv[level];
  *ptr = level_vec(s, level, which)->p;
  if (n) *n = L.n;
  return AMG_HIP_OK;
}

amg_hip_status amg_hip_sync(amg_hip_solver* s) {
  if (!s) return fail(AMG_HIP_EINVAL, "null solver");
  amg_hip_status r = set_device(s);
  if (r != AMG_HIP_OK) return r;
  HIP_TRY(hipStreamSynchronize(s->stream));
  return AMG_HIP_OK;
}

amg_hip_status amg_hip_copy_vec_dev(amg_hip_solver* s, int32_t level, int32_t which,
                                    void* dev_ptr, int32_t to_solver) {
  if (!s || !dev_ptr || level < 0 || level >= (int32_t)s->lv.size() || which < 0 || which > 2)
    return fail(AMG_HIP_EINVAL, "bad argument");
  amg_hip_status r = set_device(s);
  if (r != AMG_HIP_OK) return r;
  Level& L = s->lv[level];
  void* v = level_vec(s, level, which)->p;
  if (to_solver)
    HIP_TRY(hipMemcpyAsync(v, dev_ptr, sizeof(double) * L.n, hipMemcpyDeviceToDevice, s->stream));
  else
    HIP_TRY(hipMemcpyAsync(dev_ptr, v, sizeof(double) * L.n, hipMemcpyDeviceToDevice, s->stream));
  return AMG_HIP_OK;
}

amg_hip_status amg_hip_zero_vec(amg_hip_solver* s, int32_t level, int32_t which) {
  if (!s || level < 0 || level >= (int32_t)s->lv.size() || which < 0 || which > 2)
    return fail(AMG_HIP_EINVAL, "bad argument");
  amg_hip_status r = set_device(s);
  if (r != AMG_HIP_OK) return r;
  Level& L = s->lv[level];
  void* v = level_vec(s, level, which)->p;
  HIP_TRY(hipMemsetAsync(v, 0, sizeof(double) * L.n, s->stream));
  return AMG_HIP_OK;
}

amg_hip_status amg_hip_level_op(amg_hip_solver* s, int32_t level, int32_t op) {
  if (!s) return fail(AMG_HIP_EINVAL, "null solver");
  const int nl = (int)s->lv.size();
  if (level < 0 || level >= nl) return fail(AMG_HIP_EINVAL, "level out of range");
  amg_hip_status r = set_device(s);
  if (r != AMG_HIP_OK) return r;
  // on the solution where it rests (set_vec put it there, get_vec looks there); the bytes counted are dropped
  StepCtx X{s->stream};
  const CyclePlan P = current_plan(s);
  const LevelVecs v = resting(s, P, level);
  if ((op == 2 || op == 3) && level + 1 >= nl) return fail(AMG_HIP_EINVAL, "no coarser level");
  switch (op) {
    case 0: return enqueue_smooth(X, s, level, v);
    case 1: return enqueue_residual(X, s, level, v.u);
    case 2: return enqueue_restrict(X, s, level, resting(s, P, level + 1).u);
    case 3: return enqueue_prolong_add(X, s, level, resting(s, P, level + 1).u, v.u, v.u);
    case 4:
      if (level != nl - 1) return fail(AMG_HIP_EINVAL, "the direct solve belongs to the coarsest level");
      HIP_TRY(launch_coarse(s->coarse, s->lv[level].f.as<double>(), v.tmp, v.u, X.st));
      return AMG_HIP_OK;
  }
  return fail(AMG_HIP_EINVAL, "unknown level operation");
}

amg_hip_status amg_hip_cheb_bounds(const amg_hip_solver* s, int32_t level, double* lo, double* hi) {
  if (!s || !lo || !hi) return fail(AMG_HIP_EINVAL, "null argument");
  if (s->opt.smoother != AMG_HIP_SM_CHEBYSHEV)
    return fail(AMG_HIP_EINVAL, "amg_hip_cheb_bounds: the solver's smoother is not AMG_HIP_SM_CHEBYSHEV");
  if (level < 0 || level >= (int)s->lv.size()) return fail(AMG_HIP_EINVAL, "level out of range");
  *lo = s->lv[level].cheb_lo;
  *hi = s->lv[level].cheb_hi;
  return AMG_HIP_OK;
}

amg_hip_status amg_hip_line_stride(const amg_hip_solver* s, int32_t level, int64_t* stride) {
  if (!s || !stride) return fail(AMG_HIP_EINVAL, "null argument");
  if (s->opt.smoother != AMG_HIP_SM_LINE_JACOBI)
    return fail(AMG_HIP_EINVAL, "amg_hip_line_stride: the solver's smoother is not AMG_HIP_SM_LINE_JACOBI");
  if (level < 0 || level >= (int)s->lv.size()) return fail(AMG_HIP_EINVAL, "level out of range");
  *stride = s->lv[level].line.s;
  return AMG_HIP_OK;
}

amg_hip_status amg_hip_line_directions(const amg_hip_solver* s, int32_t level, int32_t* n_dir, int64_t strides[3]) {
  if (!s || !n_dir || !strides) return fail(AMG_HIP_EINVAL, "null argument");
  if (s->opt.smoother != AMG_HIP_SM_LINE_ALT)
    return fail(AMG_HIP_EINVAL, "amg_hip_line_directions: the solver's smoother is not AMG_HIP_SM_LINE_ALT");
  if (level < 0 || level >= (int)s->lv.size()) return fail(AMG_HIP_EINVAL, "level out of range");
  const AltOnDev& D = s->lv[level].alt;
  *n_dir = D.n_dir;
  for (int d = 0; d < 3; ++d) strides[d] = d < D.n_dir ? D.stride[d] : 0;
  return AMG_HIP_OK;
}

amg_hip_status amg_hip_line_cyclic(const amg_hip_solver* s, int32_t level, int32_t* axis_mask) {
  if (!s || !axis_mask) return fail(AMG_HIP_EINVAL, "null argument");
  if (s->opt.smoother != AMG_HIP_SM_LINE_ALT)
    return fail(AMG_HIP_EINVAL, "amg_hip_line_cyclic: the solver's smoother is not AMG_HIP_SM_LINE_ALT");
  if (level < 0 || level >= (int)s->lv.size()) return fail(AMG_HIP_EINVAL, "level out of range");
  *axis_mask = s->lv[level].alt.cyclic_mask();
  return AMG_HIP_OK;
}

amg_hip_status amg_hip_rss(amg_hip_solver* s, double* out) {
  if (!s || !out) return fail(AMG_HIP_EINVAL, "null argument");
  amg_hip_status r = set_device(s);
  if (r != AMG_HIP_OK) return r;
  Level& L = s->lv[0];
  HIP_TRY(launch_mat(CSR_RSSQ, L.A_rows, L.u.as<double>(), L.f.as<double>(), L.tmp.as<double>(),
                     1.0, s->stream));
  double* sc = s->scratch.as<double>();
  HIP_TRY(launch_sum(L.n, L.tmp.as<double>(), sc + 1024, sc, 0, s->stream));
  HIP_TRY(hipMemcpyAsync(out, sc + 1024, sizeof(double), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return AMG_HIP_OK;
}

// z = M^-1 v: one V-cycle from a zero guess on the right-hand side v (README.md:127, ref [7]
// of the reference: "a single V-cycle used for preconditioner").  Level 0's f and u are the
// cycle's operands, so they are parked in the PCG work vectors and put back.
static amg_hip_status pcg_alloc(amg_hip_solver* s) {
  const size_t bytes = sizeof(double) * (size_t)s->lv[0].n;
  if (s->pcg_x.p) return AMG_HIP_OK;
  HIP_TRY(s->pcg_x.alloc(bytes));
  HIP_TRY(s->pcg_p.alloc(bytes));
  HIP_TRY(s->pcg_q.alloc(bytes));
  HIP_TRY(s->pcg_b.alloc(bytes));
  return AMG_HIP_OK;
}
amg_hip_status amg_hip_apply(amg_hip_solver* s, const double* v_dev, double* z_dev) {
  if (!s || !v_dev || !z_dev) return fail(AMG_HIP_EINVAL, "null argument");
  amg_hip_status r = set_device(s);
  if (r != AMG_HIP_OK) return r;
  if ((r = pcg_alloc(s)) != AMG_HIP_OK) return r;
  Level& L = s->lv[0];
  const size_t bytes = sizeof(double) * (size_t)L.n;
  hipStream_t st = s->stream;
  HIP_TRY(hipMemcpyAsync(s->pcg_b.p, L.f.p, bytes, hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipMemcpyAsync(s->pcg_x.p, L.u.p, bytes, hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipMemcpyAsync(L.f.p, v_dev, bytes, hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipMemsetAsync(L.u.p, 0, bytes, st));
  if ((r = amg_hip_vcycles(s, 1)) != AMG_HIP_OK) return r;
  HIP_TRY(hipMemcpyAsync(z_dev, L.u.p, bytes, hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipMemcpyAsync(L.f.p, s->pcg_b.p, bytes, hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipMemcpyAsync(L.u.p, s->pcg_x.p, bytes, hipMemcpyDeviceToDevice, st));
  return AMG_HIP_OK;
}

// Preconditioned conjugate gradients on A_0 x = b, M^-1 = one V-cycle from zero.  During the
// iteration level 0's f holds the residual r and level 0's u receives z = M^-1 r (no copies
// around the cycle); x, p, q = A p live in the work vectors.  Start: x = the level-0
// solution; on return it holds the result and f is b again.
// The iteration shared by amg_hip_pcg and amg_hip_pcg_mixed.  r: where the residual lives, z: where
// precond() leaves M^-1 r (enqueued on the solver's stream).  b is taken from level 0's f and parked
// while r may be that very vector; x starts as level 0's u and is copied back there at the end.
// With s->project_mean (K-Center; centre(v) = v - sum(v) / n): the right-hand side of the iteration is
// centre(b), formed in q, which is free until the first q = A p; every z is centred in the pass that
// forms r . z; x is centred on every way out.  Without it the launches are the ones listed here.
extern "C++" template <class Precond>
static amg_hip_status pcg_run(amg_hip_solver* s, double rtol, int64_t max_iters, int64_t* iters, double* relres,
                              double* r, double* z, Precond precond) {
  Level& L = s->lv[0];
  const int64_t n = L.n;
  const size_t bytes = sizeof(double) * (size_t)n;
  hipStream_t st = s->stream;
  double* x = s->pcg_x.as<double>();
  double* p = s->pcg_p.as<double>();
  double* q = s->pcg_q.as<double>();
  double* bsv = s->pcg_b.as<double>();
  double* sc = s->scratch.as<double>();
  double* part = sc;              // 1024 partials
  double* d_rz = sc + 1030;       // device scalars: r.z, p.q, new r.z, r.r
  double* d_pq = sc + 1031;
  double* d_rzn = sc + 1032;
  double* d_rr = sc + 1033;
  double* d_sum = sc + 1034;      // K-Center: the sum of the vector being centred
  const bool project = s->project_mean;
  double h[2];
  // b . b
  const double* b = L.f.as<double>();
  if (project) {
    HIP_TRY(launch_sum(n, b, d_sum, part, 0, st));
    HIP_TRY(launch_center(n, d_sum, b, q, st));
    b = q;
  }
  HIP_TRY(launch_dot(n, b, b, d_rr, part, st));
  HIP_TRY(hipMemcpyAsync(h, d_rr, sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const double bnorm = std::sqrt(h[0]);
  HIP_TRY(hipMemcpyAsync(bsv, L.f.p, bytes, hipMemcpyDeviceToDevice, st));   // park b
  HIP_TRY(hipMemcpyAsync(x, L.u.p, bytes, hipMemcpyDeviceToDevice, st));     // x = u_0
  // r = b - A x (multigrid.hpp:272-274 arithmetic), in place of b
  HIP_TRY(launch_mat(CSR_RESID, L.A_rows, x, project ? q : bsv, r, 1.0, st));
  int64_t it = 0;
  double rel = 0.0;
  auto finish = [&]() -> amg_hip_status {
    if (project) {
      HIP_TRY(launch_sum(n, x, d_sum, part, 0, st));
      HIP_TRY(launch_center(n, d_sum, x, x, st));
    }
    HIP_TRY(hipMemcpyAsync(L.f.p, bsv, bytes, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(L.u.p, x, bytes, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (iters) *iters = it;
    if (relres) *relres = rel;
    return AMG_HIP_OK;
  };
  HIP_TRY(launch_dot(n, r, r, d_rr, part, st));
  HIP_TRY(hipMemcpyAsync(h, d_rr, sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  rel = bnorm > 0 ? std::sqrt(h[0]) / bnorm : std::sqrt(h[0]);
  if (rel <= rtol || max_iters == 0) return finish();
  // z = M^-1 r; p = z; rz = r . z
  amg_hip_status rc = precond();
  if (rc != AMG_HIP_OK) return rc;
  if (project) {  // z = centre(z) ahead of p = z
    HIP_TRY(launch_sum(n, z, d_sum, part, 0, st));
    HIP_TRY(launch_center_dot(n, d_sum, z, r, d_rz, part, st));
    HIP_TRY(hipMemcpyAsync(p, z, bytes, hipMemcpyDeviceToDevice, st));
  } else {
    HIP_TRY(hipMemcpyAsync(p, z, bytes, hipMemcpyDeviceToDevice, st));
    HIP_TRY(launch_dot(n, r, z, d_rz, part, st));
  }
  while (it < max_iters) {
    HIP_TRY(launch_mat(CSR_SPMV, L.A_rows, p, nullptr, q, 1.0, st));     // q = A p
    HIP_TRY(launch_dot(n, p, q, d_pq, part, st));
    HIP_TRY(launch_pcg_update_xr(n, d_rz, d_pq, x, r, p, q, st));        // alpha = rz / pq
    HIP_TRY(launch_dot(n, r, r, d_rr, part, st));
    HIP_TRY(hipMemcpyAsync(h, d_rr, sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    it += 1;
    rel = bnorm > 0 ? std::sqrt(h[0]) / bnorm : std::sqrt(h[0]);
    if (!(rel > rtol) || it >= max_iters) break;                         // NaN leaves too
    if ((rc = precond()) != AMG_HIP_OK) return rc;                       // z = M^-1 r
    if (project) {
      HIP_TRY(launch_sum(n, z, d_sum, part, 0, st));
      HIP_TRY(launch_center_dot(n, d_sum, z, r, d_rzn, part, st));
    } else {
      HIP_TRY(launch_dot(n, r, z, d_rzn, part, st));
    }
    HIP_TRY(launch_pcg_update_p(n, d_rzn, d_rz, p, z, st));              // beta = rz_new / rz
    HIP_TRY(hipMemcpyAsync(d_rz, d_rzn, sizeof(double), hipMemcpyDeviceToDevice, st));
  }
  return finish();
}

amg_hip_status amg_hip_pcg(amg_hip_solver* s, double rtol, int64_t max_iters, int64_t* iters,
                           double* relres) {
  if (!s) return fail(AMG_HIP_EINVAL, "null solver");
  if (!(rtol >= 0) || max_iters < 0) return fail(AMG_HIP_EINVAL, "bad tolerance / iteration limit");
  amg_hip_status st0 = set_device(s);
  if (st0 != AMG_HIP_OK) return st0;
  if ((st0 = pcg_alloc(s)) != AMG_HIP_OK) return st0;
  Level& L = s->lv[0];
  // the residual lives where the cycle expects its right-hand side, and the cycle leaves M^-1 r in u
  return pcg_run(s, rtol, max_iters, iters, relres, L.f.as<double>(), L.u.as<double>(), [s, &L]() -> amg_hip_status {
    HIP_TRY(hipMemsetAsync(L.u.p, 0, sizeof(double) * (size_t)L.n, s->stream));
    return amg_hip_vcycles(s, 1);
  });
}

// ---- mean projection (K-Center): the switch of the PCG drivers, and centre() on a level vector ----
amg_hip_status amg_hip_set_mean_projection(amg_hip_solver* s, int32_t on) {
  if (!s) return fail(AMG_HIP_EINVAL, "null solver");
  if (on != 0 && on != 1)
    return fail(AMG_HIP_EINVAL, "amg_hip_set_mean_projection: `on` must be 0 or 1, got " + std::to_string(on));
  if (on && !s->opt.singular)
    return fail(AMG_HIP_EINVAL, "amg_hip_set_mean_projection: the solver was not created with `singular` = 1 (the "
                                "constants are not the null space of its operator)");
  s->project_mean = on != 0;
  return AMG_HIP_OK;
}
amg_hip_status amg_hip_get_mean_projection(const amg_hip_solver* s, int32_t* on) {
  if (!s || !on) return fail(AMG_HIP_EINVAL, "null argument");
  *on = s->project_mean ? 1 : 0;
  return AMG_HIP_OK;
}
amg_hip_status amg_hip_center_vec(amg_hip_solver* s, int32_t level, int32_t which) {
  if (!s) return fail(AMG_HIP_EINVAL, "null solver");
  if (level < 0 || level >= (int32_t)s->lv.size()) return fail(AMG_HIP_EINVAL, "level out of range");
  if (which != 0 && which != 1)
    return fail(AMG_HIP_EINVAL, "amg_hip_center_vec: `which` must be 0 (u) or 1 (f), got " + std::to_string(which));
  if (s->opt.host_only) return fail(AMG_HIP_EINVAL, "host_only solver has no vectors");
  HIP_TRY(hipSetDevice(s->device));
  double* v = level_vec(s, level, which)->as<double>();
  double* sc = s->scratch.as<double>();
  const int64_t n = s->lv[level].n;
  HIP_TRY(launch_sum(n, v, sc + 1034, sc, 0, s->stream));
  HIP_TRY(launch_center(n, sc + 1034, v, v, s->stream));
  return AMG_HIP_OK;
}

// ---- single-precision preconditioner (include/amg_hip.h) ------------------------------------
amg_hip_status amg_hip_apply_f32(amg_hip_solver* s, const double* v_dev, double* z_dev) {
  if (!s || !v_dev || !z_dev) return fail(AMG_HIP_EINVAL, "null argument");
  amg_hip_status r = f32_supported(s);
  if (r != AMG_HIP_OK) return r;
  if ((r = ensure_f32(s)) != AMG_HIP_OK) return r;
  return f32_apply(s, v_dev, z_dev);
}

// r and z are ordinary device vectors of this path: level 0's f stays b and its u the start vector
// until the result replaces it
amg_hip_status amg_hip_pcg_mixed(amg_hip_solver* s, double rtol, int64_t max_iters, int64_t* iters,
                                 double* relres) {
  if (!s) return fail(AMG_HIP_EINVAL, "null solver");
  if (!(rtol >= 0) || max_iters < 0) return fail(AMG_HIP_EINVAL, "bad tolerance / iteration limit");
  amg_hip_status st0 = f32_supported(s);
  if (st0 != AMG_HIP_OK) return st0;
  if ((st0 = ensure_f32(s)) != AMG_HIP_OK) return st0;
  if ((st0 = pcg_alloc(s)) != AMG_HIP_OK) return st0;
  F32& F = s->f32;
  if (!F.pr.p) {
    const size_t bytes = sizeof(double) * (size_t)s->lv[0].n;
    HIP_TRY(F.pr.alloc(bytes));
    HIP_TRY(F.pz.alloc(bytes));
  }
  double* r = F.pr.as<double>();
  double* z = F.pz.as<double>();
  return pcg_run(s, rtol, max_iters, iters, relres, r, z, [s, r, z]() { return f32_apply(s, r, z); });
}

amg_hip_status amg_hip_f32_must_move(amg_hip_solver* s, double* bytes) {
  if (!s || !bytes) return fail(AMG_HIP_EINVAL, "null argument");
  amg_hip_status r = f32_supported(s);
  if (r != AMG_HIP_OK) return r;
  if ((r = ensure_f32(s)) != AMG_HIP_OK) return r;
  StepCtx X{s->stream, false};
  if ((r = enqueue_f32_vcycle(s, X)) != AMG_HIP_OK) return r;
  *bytes = X.once + 24.0 * (double)s->lv[0].n;  // v -> float and float -> z: 8 + 4 bytes per row each
  return AMG_HIP_OK;
}

// ---- test hooks on the float cycle (include/amg_hip.h) ---------------------------------------
// the float vector `which` of `level`, or null: the coarsest level has u and f only
static DevMem* f32_pick_vec(amg_hip_solver* s, int32_t level, int32_t which) {
  F32Level& Q = s->f32.lv[(size_t)level];
  if (which == 0) return &Q.u;
  if (which == 1) return &Q.f;
  return (which == 2 && level + 1 < (int32_t)s->lv.size()) ? &Q.r : nullptr;
}
// the checks shared by the three hooks: bad arguments (`bad`: what else is wrong with them, or null),
// then amg_hip_apply_f32's, then the float copies
static amg_hip_status f32_hook_ready(amg_hip_solver* s, int32_t level, const char* bad) {
  if (!s) return fail(AMG_HIP_EINVAL, "null solver");
  if (level < 0 || level >= (int32_t)s->lv.size()) return fail(AMG_HIP_EINVAL, "level out of range");
  if (bad) return fail(AMG_HIP_EINVAL, bad);
  amg_hip_status r = f32_supported(s);
  if (r != AMG_HIP_OK) return r;
  return ensure_f32(s);
}
static const char* f32_vec_error(const amg_hip_solver* s, int32_t level, int32_t which, const void* host) {
  if (!host) return "null argument";
  if (which < 0 || which > 2) return "bad vector selector";
  if (s && which == 2 && level + 1 == (int32_t)s->lv.size())
    return "the coarsest level of the single-precision cycle has no residual vector";
  return nullptr;
}

amg_hip_status amg_hip_f32_get_vec(amg_hip_solver* s, int32_t level, int32_t which, float* out_host) {
  amg_hip_status r = f32_hook_ready(s, level, f32_vec_error(s, level, which, out_host));
  if (r != AMG_HIP_OK) return r;
  DevMem* m = f32_pick_vec(s, level, which);
  HIP_TRY(hipStreamSynchronize(s->stream));
  HIP_TRY(hipMemcpy(out_host, m->p, sizeof(float) * (size_t)s->lv[level].n, hipMemcpyDeviceToHost));
  return AMG_HIP_OK;
}

amg_hip_status amg_hip_f32_set_vec(amg_hip_solver* s, int32_t level, int32_t which, const float* in_host) {
  amg_hip_status r = f32_hook_ready(s, level, f32_vec_error(s, level, which, in_host));
  if (r != AMG_HIP_OK) return r;
  DevMem* m = f32_pick_vec(s, level, which);
  HIP_TRY(hipStreamSynchronize(s->stream));
  HIP_TRY(hipMemcpy(m->p, in_host, sizeof(float) * (size_t)s->lv[level].n, hipMemcpyHostToDevice));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return AMG_HIP_OK;
}

amg_hip_status amg_hip_f32_level_op(amg_hip_solver* s, int32_t level, int32_t op) {
  const char* bad = nullptr;
  if (s) {
    const int32_t nl = (int32_t)s->lv.size();
    if (op < 0 || op > 4) bad = "unknown level operation";
    else if (op == 4 && level != nl - 1) bad = "the direct solve belongs to the coarsest level";
    else if (op < 4 && level + 1 >= nl)  // the coarsest level has no float matrix and no transfers
      bad = "no coarser level: the coarsest level only takes the direct solve";
  }
  amg_hip_status r = f32_hook_ready(s, level, bad);
  if (r != AMG_HIP_OK) return r;
  StepCtx X{s->stream};
  F32Steps S{s, X};
  switch (op) {
    case 0: return S.smooth(level, false);
    case 1: return S.residual(level);
    case 2: return S.restriction(level);
    case 3: return S.prolong(level);
    default: return S.coarse();
  }
}

// the checks of the two line hooks after f32_hook_ready's: a line smoother, a level with a float matrix
static amg_hip_status f32_line_hook_ready(amg_hip_solver* s, int32_t level, const char* bad) {
  amg_hip_status r = f32_hook_ready(s, level, bad);
  if (r != AMG_HIP_OK) return r;
  if (s->opt.smoother != AMG_HIP_SM_LINE_JACOBI && s->opt.smoother != AMG_HIP_SM_LINE_ALT)
    return fail(AMG_HIP_EINVAL, "the solver has no line smoother");
  if (!s->f32.lv[(size_t)level].rows.src)  // the coarsest level in the dictionary layout
    return fail(AMG_HIP_EINVAL, "level " + std::to_string(level) + " has no float matrix");
  return AMG_HIP_OK;
}

amg_hip_status amg_hip_f32_line_subsweep(amg_hip_solver* s, int32_t level, int32_t d, int32_t reverse) {
  (void)reverse;  // a sub-sweep is one direction: the leg only orders them
  amg_hip_status r = f32_line_hook_ready(s, level, d < 0 || d > 2 ? "direction index out of range" : nullptr);
  if (r != AMG_HIP_OK) return r;
  if (d >= line_dirs(s->opt.smoother, s->lv[level].alt)) return fail(AMG_HIP_EINVAL, "direction index out of range");
  StepCtx X{s->stream};
  return F32Steps{s, X}.line_subsweep(level, d);
}

amg_hip_status amg_hip_f32_line_factors(amg_hip_solver* s, int32_t level, float* dl, float* ip, float* cp) {
  amg_hip_status r = f32_line_hook_ready(s, level, !dl || !ip || !cp ? "null argument" : nullptr);
  if (r != AMG_HIP_OK) return r;
  const AltOnDev& D = s->lv[level].alt;
  if (s->opt.smoother != AMG_HIP_SM_LINE_ALT || D.n_dir == 0 || D.axis[0] != 0)
    return fail(AMG_HIP_EINVAL, "level " + std::to_string(level) + " has no x direction (K-LineX factors)");
  F32Level& Q = s->f32.lv[(size_t)level];
  const size_t bytes = sizeof(float) * (size_t)D.n;
  HIP_TRY(hipStreamSynchronize(s->stream));
  HIP_TRY(hipMemcpy(dl, Q.xdl.p, bytes, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(ip, Q.xip.p, bytes, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(cp, Q.xcp.p, bytes, hipMemcpyDeviceToHost));
  return AMG_HIP_OK;
}

amg_hip_status amg_hip_solve(amg_hip_solver* s, double tol, int64_t every, int64_t n_iters,
                             int64_t* iters, double* last_rss, int32_t* converged) {
  if (!s) return fail(AMG_HIP_EINVAL, "null solver");
  if (every > n_iters)  // multigrid.hpp:165-171
    return fail(AMG_HIP_EINVAL, "`compute_error_every_n_iters` must be leq to `n_iters`, got " +
                                    std::to_string(every) + " and " + std::to_string(n_iters));
  if (every <= 0) return fail(AMG_HIP_EINVAL, "`compute_error_every_n_iters` must be positive");
  int64_t iter = 0;
  double error = 100;  // multigrid.hpp:313
  while (iter < n_iters && error > tol) {
    // `error` only changes at the multiples of `every`: the cycles up to the next one (or to n_iters)
    // run as one call, so that they meet at their seams (amg_hip_vcycles)
    const int64_t k = std::min<int64_t>(std::min(every - iter % every, n_iters - iter), 1 << 20);
    amg_hip_status r = amg_hip_vcycles(s, (int32_t)k);
    if (r != AMG_HIP_OK) return r;
    iter += k;
    if ((iter % every) == 0) {
      if ((r = amg_hip_rss(s, &error)) != AMG_HIP_OK) return r;
    }
  }
  HIP_TRY(hipStreamSynchronize(s->stream));
  if (iters) *iters = iter;
  if (last_rss) *last_rss = error;
  if (converged) *converged = error <= tol;
  return AMG_HIP_OK;
}

int32_t amg_hip_n_levels(const amg_hip_solver* s) { return s ? (int32_t)s->lv.size() : 0; }
int64_t amg_hip_get_n_dofs(const amg_hip_solver* s, int32_t level) {
  if (!s || level < 0 || level >= (int32_t)s->lv.size()) return -1;
  return s->lv[level].n;
}
int64_t amg_hip_get_level_nnz(const amg_hip_solver* s, int32_t level) {
  if (!s || level < 0 || level >= (int32_t)s->lv.size()) return -1;
  return s->lv[level].nnz_struct;
}
amg_hip_status amg_hip_get_level_matrix(const amg_hip_solver* s, int32_t level,
                                        int32_t* colptr, int32_t* rowind, double* val) {
  if (!s || level < 0 || level >= (int32_t)s->lv.size())
    return fail(AMG_HIP_EINVAL, "level out of range");
  if (!s->opt.host_only) HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(s->lv[level].ensure_host_matrix());
  const Sparse& A = s->lv[level].A_csc;
  if (colptr) std::memcpy(colptr, A.ptr.data(), sizeof(int32_t) * A.ptr.size());
  if (rowind) std::memcpy(rowind, A.idx.data(), sizeof(int32_t) * A.idx.size());
  if (val) std::memcpy(val, A.val.data(), sizeof(double) * A.val.size());
  return AMG_HIP_OK;
}
int64_t amg_hip_get_transfer_nnz(const amg_hip_solver* s, int32_t level, int32_t which) {
  if (!s || level < 0 || level + 1 >= (int32_t)s->lv.size()) return -1;
  return (which ? s->lv[level].R() : s->lv[level].P()).nnz();
}
amg_hip_status amg_hip_get_transfer(const amg_hip_solver* s, int32_t level, int32_t which,
                                    int32_t* colptr, int32_t* rowind, double* val) {
  if (!s || level < 0 || level + 1 >= (int32_t)s->lv.size())
    return fail(AMG_HIP_EINVAL, "level out of range");
  HIP_TRY(s->lv[level].ensure_axis_weights());
  const Sparse& M = which ? s->lv[level].R() : s->lv[level].P();
  if (colptr) std::memcpy(colptr, M.ptr.data(), sizeof(int32_t) * M.ptr.size());
  if (rowind) std::memcpy(rowind, M.idx.data(), sizeof(int32_t) * M.idx.size());
  if (val) std::memcpy(val, M.val.data(), sizeof(double) * M.val.size());
  return AMG_HIP_OK;
}

amg_hip_status amg_hip_get_vec(amg_hip_solver* s, int32_t level, int32_t which, double* out) {
  DevMem* m = level_vec(s, level, which);
  if (!m || !out) return fail(AMG_HIP_EINVAL, "bad level / vector selector");
  if (s->opt.host_only) return fail(AMG_HIP_EINVAL, "host_only solver has no vectors");
  if (which == 2 && !s->opt.keep_residual && !current_plan(s).lv[(size_t)level].writes_r)
    return fail(AMG_HIP_EINVAL, "the residual of this level is not kept (create the solver with "
                                "opt.keep_residual = 1)");
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipStreamSynchronize(s->stream));
  HIP_TRY(hipMemcpy(out, m->p, sizeof(double) * s->lv[level].n, hipMemcpyDeviceToHost));
  return AMG_HIP_OK;
}
amg_hip_status amg_hip_set_vec(amg_hip_solver* s, int32_t level, int32_t which,
                               const double* in) {
  DevMem* m = level_vec(s, level, which);
  if (!m || !in) return fail(AMG_HIP_EINVAL, "bad level / vector selector");
  if (s->opt.host_only) return fail(AMG_HIP_EINVAL, "host_only solver has no vectors");
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipStreamSynchronize(s->stream));
  HIP_TRY(hipMemcpy(m->p, in, sizeof(double) * s->lv[level].n, hipMemcpyHostToDevice));
  return AMG_HIP_OK;
}
int64_t amg_hip_coarse_halfbw(const amg_hip_solver* s) { return s ? s->coarse.w : -1; }
int32_t amg_hip_coarse_solve_kind(const amg_hip_solver* s) { return s ? s->coarse.kind : -1; }

namespace {
void layout_of(const DevMat& A, int32_t* layout, int64_t* matrix_stream_bytes) {
  int32_t lay;
  int64_t bytes;
  if (A.dict) {
    lay = AMG_HIP_LAYOUT_DICT;
    bytes = (A.dict_typed ? A.n_rows + 256 * 8 * A.dict_words : A.n_rows * 8 * A.dict_words) +
            (int64_t)A.dict_ntab * 12;
  } else if (A.sell) {
    lay = AMG_HIP_LAYOUT_SELL;
    bytes = A.slots * ((A.idx16 & 1) ? 10 : 12) + (A.n_rows + 63) / 64 * 8;
  } else {
    lay = AMG_HIP_LAYOUT_CSR;
    bytes = A.csr.nnz * 12 + (A.csr.n_rows + 1) * 4;
  }
  if (layout) *layout = lay;
  if (matrix_stream_bytes) *matrix_stream_bytes = bytes;
}
}  // namespace
amg_hip_status amg_hip_level_layout(const amg_hip_solver* s, int32_t level, int32_t* layout,
                                    int64_t* matrix_stream_bytes) {
  if (!s || level < 0 || level >= (int32_t)s->lv.size())
    return fail(AMG_HIP_EINVAL, "level out of range");
  if (s->opt.host_only) return fail(AMG_HIP_EINVAL, "host_only solver has no device matrices");
  layout_of(s->lv[level].A_rows, layout, matrix_stream_bytes);
  return AMG_HIP_OK;
}

amg_hip_status amg_hip_get_colors(const amg_hip_solver* s, int32_t level, int32_t* color,
                                  int32_t* n_colors) {
  if (!s || level < 0 || level >= (int32_t)s->lv.size())
    return fail(AMG_HIP_EINVAL, "level out of range");
  const Level& L = s->lv[level];
  if (L.color.empty()) return fail(AMG_HIP_EINVAL, "solver was not built with the multicolour smoother");
  if (color) std::memcpy(color, L.color.data(), sizeof(int32_t) * L.color.size());
  if (n_colors) *n_colors = L.n_colors;
  return AMG_HIP_OK;
}

amg_hip_status amg_hip_cycle_bytes(const amg_hip_solver* s, double* cycle_bytes,
                                   double* fine_sweep_bytes) {
  if (!s) return fail(AMG_HIP_EINVAL, "null solver");
  if (cycle_bytes) *cycle_bytes = s->cycle_bytes;
  if (fine_sweep_bytes) *fine_sweep_bytes = s->fine_sweep_bytes;
  return AMG_HIP_OK;
}

namespace {
// the Chebyshev step the level-0 measurement hooks run: step 1 (a middle step) when the degree has
// one (>= 3), else step 0
void cheb_profiled_step(const amg_hip_solver* s, ChebStep* out) {
  const Level& L = s->lv[0];
  const int k = s->opt.cheb_degree;
  std::vector<double> alpha, beta;
  cheb_coefs(L.cheb_lo, L.cheb_hi, k, &alpha, &beta);
  const int j = k >= 3 ? 1 : 0;
  ChebStep c;
  c.d = L.cheb_d.as<double>();
  c.alpha = alpha[(size_t)j];
  c.beta = beta[(size_t)j];
  c.first = j == 0;
  c.last = j == k - 1;
  *out = c;
}
// n timed launches on the stream, each between two events; `after` is enqueued behind them, then the
// stream is drained
amg_hip_status no_launch() { return AMG_HIP_OK; }
extern "C++" template <class After, class Launch>
amg_hip_status time_launches(hipStream_t st, int n, double* avg_ms, double* min_ms, After after, Launch launch) {
  std::vector<hipEvent_t> ev(2 * (size_t)n);
  for (auto& e : ev) HIP_TRY(hipEventCreate(&e));
  for (int i = 0; i < n; ++i) {
    HIP_TRY(hipEventRecord(ev[2 * i], st));
    AMG_TRY(launch());
    HIP_TRY(hipEventRecord(ev[2 * i + 1], st));
  }
  AMG_TRY(after());
  HIP_TRY(hipStreamSynchronize(st));
  double sum = 0, mn = 1e30;
  for (int i = 0; i < n; ++i) {
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, ev[2 * i], ev[2 * i + 1]));
    sum += ms;
    mn = std::min<double>(mn, ms);
  }
  for (auto& e : ev) (void)hipEventDestroy(e);
  if (avg_ms) *avg_ms = sum / n;
  if (min_ms) *min_ms = mn;
  return AMG_HIP_OK;
}
}  // namespace

amg_hip_status amg_hip_profile_fine_sweep(amg_hip_solver* s, int32_t n_launches,
                                          double* avg_ms, double* min_ms) {
  if (!s || n_launches < 1) return fail(AMG_HIP_EINVAL, "bad argument");
  if (s->opt.smoother != AMG_HIP_SM_JACOBI && s->opt.smoother != AMG_HIP_SM_MULTICOLOR_GS &&
      s->opt.smoother != AMG_HIP_SM_CHEBYSHEV)
    return fail(AMG_HIP_EUNSUPPORTED, "profile_fine_sweep: only for the Jacobi, multicolour and Chebyshev smoothers");
  if (s->opt.host_only) return fail(AMG_HIP_EINVAL, "host_only solver has no device matrices");
  amg_hip_status r = set_device(s);
  if (r != AMG_HIP_OK) return r;
  Level& L = s->lv[0];
  if (s->opt.smoother == AMG_HIP_SM_CHEBYSHEV) {
    // one middle step (u -> tmp, d read and written; u is not written), else step 0
    ChebStep c;
    cheb_profiled_step(s, &c);
    return time_launches(s->stream, n_launches, avg_ms, min_ms, no_launch, [&]() -> amg_hip_status {
      HIP_TRY(launch_mat_cheb(L.A_rows, L.u.as<double>(), L.f.as<double>(), L.tmp.as<double>(), c, s->stream));
      return AMG_HIP_OK;
    });
  }
  const DevMat& A = L.A_cols();
  const CyclePlan P = current_plan(s);
  const LegForm form = P.lv[0].down;  // the launch level 0 runs
  const bool mc = s->opt.smoother == AMG_HIP_SM_MULTICOLOR_GS;
  const bool mc_patch = form == LEG_MC_PATCH;
  const bool mc_strip = form == LEG_MC_STRIP;
  // multicolour, colour kernels: the launch updates u in place; keep a copy in r
  if (mc && !mc_patch && !mc_strip)
    HIP_TRY(hipMemcpyAsync(L.r.p, L.u.p, sizeof(double) * L.n, hipMemcpyDeviceToDevice, s->stream));
  // keep u: sweep u -> tmp only (u itself is never written).  With K-Patch the launch is the
  // level's whole down-leg (2 sweeps + residual + restriction + first coarse sweep); it also
  // rewrites f and tmp of level 1, which every V-cycle recomputes before use.
  const bool patch = form == LEG_PATCH;
  MarchRef MR;
  const bool march = P.lv[0].march_down;
  if (march) (void)march_fill(s, 0, level_vecs(L, false), &MR);
  // slab-sharded solver: this rank's launch, i.e. its own lines + halo only
  const bool slab = patch && s->slab.levels > 0 && s->slab.world > 1;
  // (after the launches the multicolour colour kernels' u goes back)
  auto restore = [&]() -> amg_hip_status {
    if (mc && !mc_patch && !mc_strip)
      HIP_TRY(hipMemcpyAsync(L.u.p, L.r.p, sizeof(double) * L.n, hipMemcpyDeviceToDevice, s->stream));
    return AMG_HIP_OK;
  };
  return time_launches(s->stream, n_launches, avg_ms, min_ms, restore, [&]() -> amg_hip_status {
    if (mc_patch) {  // the first launch of the level's down-leg (its colour stages): u -> tmp
      int nd = 0;
      const std::vector<McLaunch> plan = mc_plan(s, 0, &nd);
      HIP_TRY(launch_patch_rb(false, false, L.n, L.A_rows.patch_m, L.A_rows.patch_ref(), L.u.as<double>(),
                              L.f.as<double>(), nullptr, s->lv[1].n, L.tmp.as<double>(), nullptr, nullptr,
                              nullptr, plan[0].stages, (uint32_t)L.mc_ctab, s->stream));
    } else if (mc_strip) {
      // the level's whole down-leg, u -> tmp (down_mc_strip without r); like the K-Patch launch it
      // rewrites f and u of level 1, which every V-cycle recomputes before use
      Level& C = s->lv[1];
      StripRef R = mc_strip_ref(s, 0);
      R.x = L.u.as<double>();
      R.u_out = L.tmp.as<double>();
      R.fH = C.f.as<double>();
      R.uH_zero = C.u.as<double>();
      HIP_TRY(launch_mc_strip(false, true, R, L.A_rows.dict_ref(), s->stream));
    } else if (mc) {  // colour 0 of the forward half
      if (L.mc_dict)
        HIP_TRY(launch_dict_gs_color(L.mc_start[0], L.mc_start[1] - L.mc_start[0], L.mc_words, L.mc_wmax,
                                     L.mc_codes.as<uint64_t>(), L.mc_rowid.as<int32_t>(),
                                     L.mc_doff.as<int32_t>(), L.mc_dval.as<double>(), L.mc_ntab,
                                     L.f.as<double>(), L.u.as<double>(), s->stream));
      else
        HIP_TRY(launch_sell_gs_color(L.mc_mat.n_rows, L.mc_mat.max_width, L.mc_mat.soff.as<int64_t>(),
                                     L.mc_mat.scol.as<int32_t>(), L.mc_mat.sval.as<double>(),
                                     L.mc_rowid.as<int32_t>(), L.mc_start[0], L.mc_start[1] - L.mc_start[0],
                                     L.f.as<double>(), L.u.as<double>(), s->stream));
    } else if (march) {  // both sweeps of level 0 in one plane-marching pass: u -> tmp
      HIP_TRY(launch_march(MR, s->stream));
    } else if (patch) {
      Level& C = s->lv[1];
      HIP_TRY(launch_patch_down(true, L.n, A.patch_m, A.patch_ref(), L.u.as<double>(),
                                L.f.as<double>(), L.tmp.as<double>(), nullptr, C.n, C.f.as<double>(),
                                C.diag.as<double>(), P.lv[0].xf_out ? nullptr : C.tmp.as<double>(),
                                s->opt.omega, s->stream,
                                slab ? s->slab.down_lo[0] : 0, slab ? s->slab.down_hi[0] : -1));
    } else {
      HIP_TRY(launch_mat(CSR_JACOBI, A, L.u.as<double>(), L.f.as<double>(), L.tmp.as<double>(),
                         s->opt.omega, s->stream));
    }
    return AMG_HIP_OK;
  });
}

amg_hip_status amg_hip_cycle_must_move(amg_hip_solver* s, int32_t part, double* bytes) {
  if (!s || !bytes || part < 0 || part > 4) return fail(AMG_HIP_EINVAL, "bad argument");
  if (s->opt.host_only) return fail(AMG_HIP_EINVAL, "host_only solver has no device cycle");
  if (part == 4) {
    // one steady-state cycle of amg_hip_vcycles(s, n >= 2): the seam cycle where the solver runs one
    // (counted while its graph is captured), else the stand-alone cycle
    if (!current_plan(s).seam) return amg_hip_cycle_must_move(s, CYCLE_ALL, bytes);
    if (s->must_move[4] == 0.0) {
      amg_hip_status r = set_device(s);
      if (r != AMG_HIP_OK) return r;
      if (!s->opt.use_graph) return fail(AMG_HIP_EINVAL, "amg_hip_cycle_must_move: run two V-cycles in one call first");
      const int gi = 2;  // the seam cycle that reads tmp: captured, not run
      r = s->seam_graph[gi].capture(s->stream, [s] { return enqueue_vcycle(s, CYCLE_ALL, SEAM_CYCLE, 0); });
      if (r != AMG_HIP_OK) return r;
    }
    *bytes = s->must_move[4];
    return AMG_HIP_OK;
  }
  if (part == CYCLE_ALL && s->must_move[0] == 0.0 && !s->opt.window) {
    // not enqueued yet: capturing the graph walks the cycle without running it
    amg_hip_status r = set_device(s);
    if (r != AMG_HIP_OK) return r;
    if (!s->opt.use_graph) return fail(AMG_HIP_EINVAL, "amg_hip_cycle_must_move: run a V-cycle first");
    if ((r = s->graph.capture(s->stream, [s] { return enqueue_vcycle(s); })) != AMG_HIP_OK) return r;
  }
  *bytes = s->must_move[part];
  return AMG_HIP_OK;
}

int32_t amg_hip_patch_leg_lines(const amg_hip_solver* s, int32_t level, int32_t leg) {
  if (!s || s->opt.host_only || level < 0 || level >= (int32_t)s->lv.size() || leg < 0 || leg > 2) return 0;
  const CyclePlan P = current_plan(s);
  const LegForm form = P.lv[(size_t)level].up;  // (a patch level is one on both legs)
  if (leg == 2) return (level == 0 && P.seam) ? patch_seam_lines() : 0;  // the seam launch
  if (form == LEG_MC_PATCH) return patch_tile_lines(3);
  if (form != LEG_PATCH) return 0;
  return patch_tile_lines(patch_rings(s, leg == 0 && level == 0));
}

namespace {
int32_t leg_form_public(LegForm f) {
  switch (f) {
    case LEG_NONE: return AMG_HIP_LEG_NONE;
    case LEG_PLAIN: return AMG_HIP_LEG_PLAIN;
    case LEG_PAIR: return AMG_HIP_LEG_PAIR;
    case LEG_DUO_FINE: return AMG_HIP_LEG_DUO_FINE;
    case LEG_DUO_COARSE: return AMG_HIP_LEG_DUO_COARSE;
    case LEG_PATCH: return AMG_HIP_LEG_PATCH;
    case LEG_MC_PATCH: return AMG_HIP_LEG_MC_PATCH;
    case LEG_MC_STRIP: return AMG_HIP_LEG_MC_STRIP;
    case LEG_TAIL_HEAD: return AMG_HIP_LEG_TAIL_HEAD;
    case LEG_IN_TAIL: return AMG_HIP_LEG_IN_TAIL;
  }
  return AMG_HIP_LEG_NONE;
}
}  // namespace

amg_hip_status amg_hip_level_leg_form(const amg_hip_solver* s, int32_t level, int32_t* down, int32_t* up) {
  if (!s || !down || !up || level < 0 || level >= (int32_t)s->lv.size())
    return fail(AMG_HIP_EINVAL, "amg_hip_level_leg_form: bad argument");
  const CyclePlan P = current_plan(s);  // host_only: every level none
  *down = leg_form_public(P.lv[(size_t)level].down);
  *up = leg_form_public(P.lv[(size_t)level].up);
  return AMG_HIP_OK;
}

amg_hip_status amg_hip_strip_geometry(const amg_hip_solver* s, int32_t level, int32_t* T, int32_t* tiles,
                                      int32_t* stages, int32_t* halo_down, int32_t* halo_up) {
  if (!s || !T || !tiles || !stages || !halo_down || !halo_up || level < 0 || level >= (int32_t)s->lv.size())
    return fail(AMG_HIP_EINVAL, "amg_hip_strip_geometry: bad argument");
  // (a strip level is one on both legs)
  if (s->opt.host_only || current_plan(s).lv[(size_t)level].up != LEG_MC_STRIP)
    return fail(AMG_HIP_EINVAL, "amg_hip_strip_geometry: the level is no K-Strip level");
  const StripRef R = mc_strip_ref(const_cast<amg_hip_solver*>(s), level);  // reads only
  *T = R.T;
  *tiles = (R.n + R.T - 1) / R.T;
  *stages = R.nst;
  *halo_down = (R.nst + 1) * R.hbw;  // launch_mc_strip: H = (nst + tail) hbw
  *halo_up = R.nst * R.hbw;
  return AMG_HIP_OK;
}

amg_hip_status amg_hip_patch_tile_classes(amg_hip_solver* s, int32_t level, int32_t rings, int64_t* out) {
  if (!s || !out || s->opt.host_only || level < 0 || level >= (int32_t)s->lv.size())
    return fail(AMG_HIP_EINVAL, "amg_hip_patch_tile_classes: bad argument");
  if (rings != 2 && rings != 3 && rings != 5)
    return fail(AMG_HIP_EINVAL, "amg_hip_patch_tile_classes: rings is 2 (44-line tiles), 3 (42) or 5 (the seam's, 38)");
  const LegForm form = current_plan(s).lv[(size_t)level].up;  // (a patch level is one on both legs)
  const DevMat& A = s->lv[(size_t)level].A_rows;
  const DevMem& F = rings == 2 ? A.patch_flags2 : (rings == 5 ? A.patch_flags5 : A.patch_flags);
  if ((form != LEG_PATCH && form != LEG_MC_PATCH) || !A.patch || !F.p)
    return fail(AMG_HIP_EINVAL, "amg_hip_patch_tile_classes: the level is no K-Patch level (or has no tiles of this geometry)");
  int64_t tiles = 0;
  const int64_t n = s->lv[(size_t)level].n;
  const amg_hip_status r = set_device(s);
  if (r != AMG_HIP_OK) return r;
  HIP_TRY(rings == 5 ? launch_patch_seam_flags(n, A.patch_m, nullptr, A.patch_ntypes, nullptr, &tiles, nullptr)
                     : launch_patch_tile_flags(n, A.patch_m, rings, nullptr, A.patch_ntypes, nullptr, &tiles, nullptr));
  std::vector<uint8_t> fl((size_t)tiles);
  HIP_TRY(hipMemcpy(fl.data(), F.p, fl.size(), hipMemcpyDeviceToHost));
  out[0] = out[1] = out[2] = 0;
  for (uint8_t f : fl) ++out[f == 255 ? 2 : (f == 254 ? 1 : 0)];
  return AMG_HIP_OK;
}

amg_hip_status amg_hip_fine_sweep_info(const amg_hip_solver* s, char* name, int32_t name_cap,
                                       int32_t* sweeps_per_launch, double* bytes_per_launch) {
  if (!s || !name || name_cap < 32) return fail(AMG_HIP_EINVAL, "bad argument");
  if (s->opt.smoother == AMG_HIP_SM_LINE_JACOBI || s->opt.smoother == AMG_HIP_SM_LINE_ALT)
    return fail(AMG_HIP_EUNSUPPORTED, "fine_sweep_info: a line-smoother sweep is not one launch");
  if (s->opt.host_only) return fail(AMG_HIP_EINVAL, "host_only solver has no device matrices");
  const Level& L = s->lv[0];
  const DevMat& A = L.A_cols();
  const CyclePlan P = current_plan(s);
  const LevelPlan& Q = P.lv[0];  // the launch level 0 runs
  int32_t lay = 0;
  int64_t mat = 0;
  layout_of(A, &lay, &mat);
  int sweeps = 1;
  // bytes one launch has to move: what it reads and writes once, not a layout it does not stream
  double bytes = 12.0 * (double)L.nnz_struct + 28.0 * (double)L.n;  // SELL / CSR: SURVEY 8(d)
  if (s->opt.smoother == AMG_HIP_SM_CHEBYSHEV) {
    // the step amg_hip_profile_fine_sweep runs: matrix in its layout, f, x, out, d read / written
    ChebStep c;
    cheb_profiled_step(s, &c);
    const int mode = cheb_kernel_mode(c.first, c.last);
    const DevMat& R = L.A_rows;
    layout_of(R, &lay, &mat);
    if (R.dict) {
      dict_kernel_name(mode, R.n_rows, R.dict_ref(), L.f.p, L.tmp.p, name, (size_t)name_cap);
    } else if (R.sell) {
      std::snprintf(name, (size_t)name_cap, "sell_kernel<%d, %s, %s>", mode, (R.idx16 & 1) ? "true" : "false",
                    (R.idx16 & 2) ? "true" : "false");
    } else {
      std::snprintf(name, (size_t)name_cap, "csr_stage_kernel<%d>", mode);
    }
    bytes = (double)mat + 24.0 * (double)L.n + (c.first ? 0.0 : 8.0 * L.n) + (c.last ? 0.0 : 8.0 * L.n);
  } else if (s->opt.smoother == AMG_HIP_SM_MULTICOLOR_GS) {
    // one launch of the symmetric pass: two colour stages over the level (patch form), or one
    // colour of one direction (colour kernels: half the rows)
    if (Q.down == LEG_MC_PATCH) {
      std::snprintf(name, (size_t)name_cap, "patch_rb_kernel<%d, %d, %s, false, false>", patch_un(A.patch_un),
                    patch_kind_umask(A.patch_un, A.patch_umask), A.dict_nt ? "true" : "false");
      bytes = 25.0 * (double)L.n;
    } else if (Q.down == LEG_MC_STRIP) {
      // the level's whole down-leg (down_mc_strip): every colour stage of the symmetric passes, the
      // residual and the restriction: row types + colours + x + f + out; f_H, zeroed u_H
      const StripRef R = mc_strip_ref(const_cast<amg_hip_solver*>(s), 0);  // reads only
      mc_strip_kernel_name(L.A_rows.dict_ref(), false, true, name, (size_t)name_cap);
      sweeps = R.nst;
      bytes = 26.0 * (double)L.n + 16.0 * (double)s->lv[1].n;
    } else {
      std::snprintf(name, (size_t)name_cap, "%s", L.mc_dict ? "dict_gs_color_kernel" : "sell_kernel<5>");
      const double rows = (double)(L.mc_start.size() > 1 ? L.mc_start[1] - L.mc_start[0] : L.n);
      // rows of colour 0: code words + dof id (dictionary) or their share of the panels, f, u written
      bytes = L.mc_dict ? rows * (8.0 * L.mc_words + 4.0 + 16.0)
                        : rows / (double)L.n * (12.0 * (double)L.nnz_struct + 28.0 * (double)L.n);
    }
  } else if (Q.down == LEG_PATCH) {
    // row types + x + f + smoothed u per fine row; f_H and, unless level 1 forms it from f_H itself
    // (the hand-over), the first coarse sweep and the coarse diagonal
    std::snprintf(name, (size_t)name_cap, "patch_down_kernel<%d, %d, true, %s, false, 3>", patch_un(A.patch_un),
                  patch_kind_umask(A.patch_un, A.patch_umask), A.dict_nt ? "true" : "false");
    sweeps = 2;
    bytes = 25.0 * (double)L.n + (Q.xf_out ? 8.0 : 24.0 - 8.0 * A.patch_cfrac) * (double)s->lv[1].n;
    if (s->slab.levels > 0 && s->slab.world > 1) {  // the tiles this rank's launch covers
      const int64_t th = patch_tile_lines(patch_rings(s, true));  // the level-0 down-leg's tiles
      const int64_t l0 = s->slab.down_lo[0] / th * th;
      const int64_t l1 = std::min<int64_t>(s->slab.lines, (s->slab.down_hi[0] + th - 1) / th * th);
      bytes *= (double)(l1 - l0) / (double)s->slab.lines;
    }
  } else if (Q.march_down) {
    // both sweeps of the level in one pass: row types + x + f + out
    std::snprintf(name, (size_t)name_cap, "march_kernel");
    sweeps = 2;
    bytes = (double)mat + 24.0 * (double)L.n;
  } else if (A.dict) {
    dict_kernel_name(CSR_JACOBI, A.n_rows, A.dict_ref(), L.f.p, L.tmp.p, name, (size_t)name_cap);
    bytes = (double)mat + 24.0 * (double)L.n;  // matrix stream (1 B / row) + f + x + out
  } else if (A.sell) {
    std::snprintf(name, (size_t)name_cap, "sell_kernel<1, %s, %s>", (A.idx16 & 1) ? "true" : "false",
                  (A.idx16 & 2) ? "true" : "false");
  } else {
    std::snprintf(name, (size_t)name_cap, "csr_stage_kernel<1>");
  }
  if (sweeps_per_launch) *sweeps_per_launch = sweeps;
  if (bytes_per_launch) *bytes_per_launch = bytes;
  return AMG_HIP_OK;
}

// ---- stand-alone operations on host arrays -------------------------------------
amg_hip_status amg_hip_residual(int64_t n, const int32_t* colptr, const int32_t* rowind,
                                const double* val, const double* u, const double* f,
                                double* r) {
  amg_hip_status st = need_device();
  if (st != AMG_HIP_OK) return st;
  if (n <= 0 || !colptr || !rowind || !val || !u || !f || !r)
    return fail(AMG_HIP_EINVAL, "bad argument");
  Sparse A = from_raw(n, n, colptr, rowind, val);
  std::string v = validate(A, "A");
  if (!v.empty()) return fail(AMG_HIP_EINVAL, v);
  Sparse Ar = transpose(A);
  DevMat D;
  DevMem du, df, dr;
  HIP_TRY(upload_mat(Ar, g_default_layout, &D));
  HIP_TRY(upload(du, u, (size_t)n));
  HIP_TRY(upload(df, f, (size_t)n));
  HIP_TRY(dr.alloc(sizeof(double) * n));
  HIP_TRY(launch_mat(CSR_RESID, D, du.as<double>(), df.as<double>(), dr.as<double>(), 1.0, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(r, dr.p, sizeof(double) * n, hipMemcpyDeviceToHost));
  return AMG_HIP_OK;
}

amg_hip_status amg_hip_spmv(int64_t rows, int64_t cols, const int32_t* colptr,
                            const int32_t* rowind, const double* val, const double* v,
                            double* out) {
  amg_hip_status st = need_device();
  if (st != AMG_HIP_OK) return st;
  if (rows <= 0 || cols <= 0 || !colptr || !rowind || !val || !v || !out)
    return fail(AMG_HIP_EINVAL, "bad argument");
  Sparse M = from_raw(cols, rows, colptr, rowind, val);
  std::string e = validate(M, "M");
  if (!e.empty()) return fail(AMG_HIP_EINVAL, e);
  Sparse Mr = transpose(M);
  DevMat D;
  DevMem dv, dout;
  HIP_TRY(upload_mat(Mr, g_default_layout, &D));
  HIP_TRY(upload(dv, v, (size_t)cols));
  HIP_TRY(dout.alloc(sizeof(double) * rows));
  HIP_TRY(launch_mat(CSR_SPMV, D, dv.as<double>(), nullptr, dout.as<double>(), 1.0, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, dout.p, sizeof(double) * rows, hipMemcpyDeviceToHost));
  return AMG_HIP_OK;
}

amg_hip_status amg_hip_linear_restrict(int64_t n_h, int64_t n_H, const double* r, double* f_H) {
  amg_hip_status st = need_device();
  if (st != AMG_HIP_OK) return st;
  if (n_h <= 0 || n_H <= 0 || !r || !f_H) return fail(AMG_HIP_EINVAL, "bad argument");
  DevMem dr, df;
  HIP_TRY(upload(dr, r, (size_t)n_h));
  HIP_TRY(df.alloc(sizeof(double) * n_H));
  HIP_TRY(launch_linear_restrict(n_h, n_H, dr.as<double>(), df.as<double>(), nullptr, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(f_H, df.p, sizeof(double) * n_H, hipMemcpyDeviceToHost));
  return AMG_HIP_OK;
}

// the fine grid of a stand-alone tensor transfer: every coarsened axis needs 2 points.  mask < 0:
// full coarsening (the entry points without a mask)
// sides: the natural boundary sides of the _bc entry points (0 for the others)
// periodic: the periodic axes of the _per entry points (0 for the others)
static amg_hip_status tensor_transfer_args(const char* who, int32_t dim, const int64_t* dims, int64_t mask_in,
                                           int32_t sides, int32_t periodic, uint32_t* mask, int64_t* n_h,
                                           int64_t* n_H) {
  std::string e = tensor_dims_error(dim, dims);
  if (e.empty()) e = periodic_axes_error(dim, periodic);
  if (e.empty() && (sides < 0 || sides >= (1 << (2 * dim))))
    e = "`natural_sides` = " + std::to_string(sides) + " has bits other than the " + std::to_string(2 * dim) +
        " sides of the grid";
  if (e.empty() && mask_in < 0) {
    if (dims[0] < 2 || dims[1] < 2 || (dim == 3 && dims[2] < 2)) e = "an axis of fewer than 2 points cannot be coarsened";
    mask_in = tensor_full_mask(dim);
  } else if (e.empty()) {
    e = semi_mask_error(0, dim, dims, mask_in);
  }
  if (e.empty() && periodic) {
    e = periodic_level_error(0, dim, dims, (uint32_t)mask_in, (uint32_t)periodic);
    for (int a = 0; e.empty() && a < dim; ++a)
      if (((periodic >> a) & 1) && ((sides >> (2 * a)) & 3))
        e = "`natural_sides` = " + std::to_string(sides) + " names a side of axis " + std::string(1, "xyz"[a]) +
            ", which `periodic_axes` = " + std::to_string(periodic) + " makes periodic: a periodic axis has no sides";
  }
  if (!e.empty()) return fail(AMG_HIP_EINVAL, std::string(who) + ": " + e);
  int64_t c[3];
  *mask = (uint32_t)mask_in;
  tensor_coarse_dims(dim, dims, *mask, c);
  *n_h = dims[0] * dims[1] * dims[2];
  *n_H = c[0] * c[1] * c[2];
  return AMG_HIP_OK;
}

static amg_hip_status tensor_restrict_host(const char* who, int32_t dim, const int64_t* dims_h, int64_t mask_in,
                                           int32_t sides, const double* r, double* f_H, int32_t periodic = 0) {
  int64_t n_h = 0, n_H = 0;
  uint32_t mask = 0;
  amg_hip_status st = tensor_transfer_args(who, dim, dims_h, mask_in, sides, periodic, &mask, &n_h, &n_H);
  if (st != AMG_HIP_OK) return st;
  if (!r || !f_H) return fail(AMG_HIP_EINVAL, "bad argument");
  if ((st = need_device()) != AMG_HIP_OK) return st;
  DevMem dr, df;
  HIP_TRY(upload(dr, r, (size_t)n_h));
  HIP_TRY(df.alloc(sizeof(double) * n_H));
  HIP_TRY(launch_tensor_restrict(dim, dims_h, mask, (uint32_t)sides, (uint32_t)periodic, dr.as<double>(), df.as<double>(), nullptr, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(f_H, df.p, sizeof(double) * n_H, hipMemcpyDeviceToHost));
  return AMG_HIP_OK;
}
amg_hip_status amg_hip_tensor_restrict(int32_t dim, const int64_t* dims_h, const double* r, double* f_H) {
  return tensor_restrict_host("amg_hip_tensor_restrict", dim, dims_h, -1, 0, r, f_H);
}
amg_hip_status amg_hip_tensor_restrict_axes(int32_t dim, const int64_t* dims_h, int32_t axis_mask, const double* r,
                                            double* f_H) {
  return tensor_restrict_host("amg_hip_tensor_restrict_axes", dim, dims_h, axis_mask < 0 ? 8 : axis_mask, 0, r, f_H);
}
amg_hip_status amg_hip_tensor_restrict_bc(int32_t dim, const int64_t* dims_h, int32_t axis_mask, int32_t natural_sides,
                                          const double* r, double* f_H) {
  return tensor_restrict_host("amg_hip_tensor_restrict_bc", dim, dims_h, axis_mask < 0 ? 8 : axis_mask, natural_sides,
                              r, f_H);
}
amg_hip_status amg_hip_tensor_restrict_per(int32_t dim, const int64_t* dims_h, int32_t axis_mask, int32_t natural_sides,
                                           int32_t periodic_axes, const double* r, double* f_H) {
  return tensor_restrict_host("amg_hip_tensor_restrict_per", dim, dims_h, axis_mask < 0 ? 8 : axis_mask, natural_sides,
                              r, f_H, periodic_axes);
}

static amg_hip_status tensor_prolong_add_host(const char* who, int32_t dim, const int64_t* dims_h, int64_t mask_in,
                                              int32_t sides, const double* u_H, double* u_h, int32_t periodic = 0) {
  int64_t n_h = 0, n_H = 0;
  uint32_t mask = 0;
  amg_hip_status st = tensor_transfer_args(who, dim, dims_h, mask_in, sides, periodic, &mask, &n_h, &n_H);
  if (st != AMG_HIP_OK) return st;
  if (!u_H || !u_h) return fail(AMG_HIP_EINVAL, "bad argument");
  if ((st = need_device()) != AMG_HIP_OK) return st;
  DevMem dH, dh;
  HIP_TRY(upload(dH, u_H, (size_t)n_H));
  HIP_TRY(upload(dh, u_h, (size_t)n_h));
  HIP_TRY(launch_tensor_prolong_add(dim, dims_h, mask, (uint32_t)sides, (uint32_t)periodic, dH.as<double>(), dh.as<double>(), nullptr));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(u_h, dh.p, sizeof(double) * n_h, hipMemcpyDeviceToHost));
  return AMG_HIP_OK;
}
// the fine grid, the axis and the sizes of a stand-alone K-AxisRestrict / K-AxisProlong call
static amg_hip_status axis_transfer_args(const char* who, int32_t dim, const int64_t* dims, int32_t axis,
                                         int32_t periodic, int32_t vec_shift, int64_t* n_h, int64_t* n_H) {
  std::string e = tensor_dims_error(dim, dims);
  if (e.empty() && (axis < 0 || axis >= dim)) e = "`axis` must be in [0, " + std::to_string(dim) + "), got " + std::to_string(axis);
  if (e.empty()) e = semi_mask_error(0, dim, dims, (int64_t)1 << axis);
  if (e.empty() && periodic != 0 && periodic != 1) e = "`periodic` must be 0 or 1, got " + std::to_string(periodic);
  if (e.empty() && vec_shift != 0 && vec_shift != 1) e = "`vec_shift` must be 0 or 1, got " + std::to_string(vec_shift);
  if (e.empty() && periodic && (dims[axis] < 4 || (dims[axis] & 1)))
    e = "axis " + std::string(1, "xyz"[axis]) + " has " + std::to_string(dims[axis]) +
        " points; a coarsened periodic axis needs an even length of at least 4";
  if (!e.empty()) return fail(AMG_HIP_EINVAL, std::string(who) + ": " + e);
  *n_h = dims[0] * dims[1] * dims[2];
  *n_H = *n_h / dims[axis] * (dims[axis] / 2);
  return AMG_HIP_OK;
}
// periodic / vec_shift: the _per entry points (0, 0 for the others).  A vector of `len` doubles lives
// `vec_shift` doubles into an allocation of len + 1, so that it starts 8 bytes past a 16-byte boundary.
static amg_hip_status axis_restrict_host(const char* who, int32_t dim, const int64_t* dims, int32_t axis,
                                         int32_t periodic, const double* W, const double* r, double* f_H,
                                         int32_t vec_shift) {
  int64_t n_h = 0, n_H = 0;
  amg_hip_status st = axis_transfer_args(who, dim, dims, axis, periodic, vec_shift, &n_h, &n_H);
  if (st != AMG_HIP_OK) return st;
  if (!W || !r || !f_H) return fail(AMG_HIP_EINVAL, "bad argument");
  if ((st = need_device()) != AMG_HIP_OK) return st;
  DevMem dw, dr, df;
  HIP_TRY(upload(dw, W, (size_t)(2 * (n_h - n_H))));
  HIP_TRY(dr.alloc(sizeof(double) * (n_h + 1)));
  HIP_TRY(df.alloc(sizeof(double) * (n_H + 1)));
  double* rd = dr.as<double>() + vec_shift;
  double* fd = df.as<double>() + vec_shift;
  HIP_TRY(hipMemcpy(rd, r, sizeof(double) * n_h, hipMemcpyHostToDevice));
  HIP_TRY(launch_axis_restrict(dim, dims, axis, periodic != 0, dw.as<double>(), rd, fd, nullptr, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(f_H, fd, sizeof(double) * n_H, hipMemcpyDeviceToHost));
  return AMG_HIP_OK;
}
static amg_hip_status axis_prolong_add_host(const char* who, int32_t dim, const int64_t* dims, int32_t axis,
                                            int32_t periodic, const double* W, const double* u_H, double* u_h,
                                            int32_t vec_shift) {
  int64_t n_h = 0, n_H = 0;
  amg_hip_status st = axis_transfer_args(who, dim, dims, axis, periodic, vec_shift, &n_h, &n_H);
  if (st != AMG_HIP_OK) return st;
  if (!W || !u_H || !u_h) return fail(AMG_HIP_EINVAL, "bad argument");
  if ((st = need_device()) != AMG_HIP_OK) return st;
  DevMem dw, dH, dh;
  HIP_TRY(upload(dw, W, (size_t)(2 * (n_h - n_H))));
  HIP_TRY(dH.alloc(sizeof(double) * (n_H + 1)));
  HIP_TRY(dh.alloc(sizeof(double) * (n_h + 1)));
  double* Hd = dH.as<double>() + vec_shift;
  double* hd = dh.as<double>() + vec_shift;
  HIP_TRY(hipMemcpy(Hd, u_H, sizeof(double) * n_H, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(hd, u_h, sizeof(double) * n_h, hipMemcpyHostToDevice));
  HIP_TRY(launch_axis_prolong_add(dim, dims, axis, periodic != 0, dw.as<double>(), Hd, hd, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(u_h, hd, sizeof(double) * n_h, hipMemcpyDeviceToHost));
  return AMG_HIP_OK;
}
amg_hip_status amg_hip_axis_restrict(int32_t dim, const int64_t* dims, int32_t axis, const double* W, const double* r,
                                     double* f_H) {
  return axis_restrict_host("amg_hip_axis_restrict", dim, dims, axis, 0, W, r, f_H, 0);
}
amg_hip_status amg_hip_axis_prolong_add(int32_t dim, const int64_t* dims, int32_t axis, const double* W,
                                        const double* u_H, double* u_h) {
  return axis_prolong_add_host("amg_hip_axis_prolong_add", dim, dims, axis, 0, W, u_H, u_h, 0);
}
amg_hip_status amg_hip_axis_restrict_per(int32_t dim, const int64_t* dims, int32_t axis, int32_t periodic,
                                         const double* W, const double* r, double* f_H, int32_t vec_shift) {
  return axis_restrict_host("amg_hip_axis_restrict_per", dim, dims, axis, periodic, W, r, f_H, vec_shift);
}
amg_hip_status amg_hip_axis_prolong_add_per(int32_t dim, const int64_t* dims, int32_t axis, int32_t periodic,
                                            const double* W, const double* u_H, double* u_h, int32_t vec_shift) {
  return axis_prolong_add_host("amg_hip_axis_prolong_add_per", dim, dims, axis, periodic, W, u_H, u_h, vec_shift);
}

amg_hip_status amg_hip_tensor_prolong_add(int32_t dim, const int64_t* dims_h, const double* u_H,
                                          double* u_h) {
  return tensor_prolong_add_host("amg_hip_tensor_prolong_add", dim, dims_h, -1, 0, u_H, u_h);
}
amg_hip_status amg_hip_tensor_prolong_add_axes(int32_t dim, const int64_t* dims_h, int32_t axis_mask,
                                               const double* u_H, double* u_h) {
  return tensor_prolong_add_host("amg_hip_tensor_prolong_add_axes", dim, dims_h, axis_mask < 0 ? 8 : axis_mask, 0,
                                 u_H, u_h);
}
amg_hip_status amg_hip_tensor_prolong_add_bc(int32_t dim, const int64_t* dims_h, int32_t axis_mask,
                                             int32_t natural_sides, const double* u_H, double* u_h) {
  return tensor_prolong_add_host("amg_hip_tensor_prolong_add_bc", dim, dims_h, axis_mask < 0 ? 8 : axis_mask,
                                 natural_sides, u_H, u_h);
}
amg_hip_status amg_hip_tensor_prolong_add_per(int32_t dim, const int64_t* dims_h, int32_t axis_mask,
                                              int32_t natural_sides, int32_t periodic_axes, const double* u_H,
                                              double* u_h) {
  return tensor_prolong_add_host("amg_hip_tensor_prolong_add_per", dim, dims_h, axis_mask < 0 ? 8 : axis_mask,
                                 natural_sides, u_H, u_h, periodic_axes);
}

amg_hip_status amg_hip_linear_prolong_add(int64_t n_h, int64_t n_H, const double* u_H,
                                          double* u_h) {
  amg_hip_status st = need_device();
  if (st != AMG_HIP_OK) return st;
  if (n_h <= 0 || n_H <= 0 || !u_H || !u_h) return fail(AMG_HIP_EINVAL, "bad argument");
  DevMem dH, dh;
  HIP_TRY(upload(dH, u_H, (size_t)n_H));
  HIP_TRY(upload(dh, u_h, (size_t)n_h));
  HIP_TRY(launch_linear_prolong_add(n_h, n_H, dH.as<double>(), dh.as<double>(), nullptr));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(u_h, dh.p, sizeof(double) * n_h, hipMemcpyDeviceToHost));
  return AMG_HIP_OK;
}

amg_hip_status amg_hip_rss_host(int64_t n, const int32_t* colptr, const int32_t* rowind,
                                const double* val, const double* u, const double* b,
                                double* out) {
  amg_hip_status st = need_device();
  if (st != AMG_HIP_OK) return st;
  if (n <= 0 || !colptr || !rowind || !val || !u || !b || !out)
    return fail(AMG_HIP_EINVAL, "bad argument");
  Sparse A = from_raw(n, n, colptr, rowind, val);
  std::string v = validate(A, "A");
  if (!v.empty()) return fail(AMG_HIP_EINVAL, v);
  Sparse Ar = transpose(A);
  DevMat D;
  DevMem du, db, dt, sc;
  HIP_TRY(upload_mat(Ar, g_default_layout, &D));
  HIP_TRY(upload(du, u, (size_t)n));
  HIP_TRY(upload(db, b, (size_t)n));
  HIP_TRY(dt.alloc(sizeof(double) * n));
  HIP_TRY(sc.alloc(sizeof(double) * 1100));
  HIP_TRY(launch_mat(CSR_RSSQ, D, du.as<double>(), db.as<double>(), dt.as<double>(), 1.0, nullptr));
  HIP_TRY(launch_sum(n, dt.as<double>(), sc.as<double>() + 1024, sc.as<double>(), 0, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, sc.as<double>() + 1024, sizeof(double), hipMemcpyDeviceToHost));
  return AMG_HIP_OK;
}

amg_hip_status amg_hip_coarse_solve(int64_t n, const int32_t* colptr, const int32_t* rowind,
                                    const double* val, const double* f, double* x,
                                    int64_t* halfbw) {
  amg_hip_status st = need_device();
  if (st != AMG_HIP_OK) return st;
  if (n <= 0 || !colptr || !rowind || !val || !f || !x) return fail(AMG_HIP_EINVAL, "bad argument");
  Sparse A = from_raw(n, n, colptr, rowind, val);
  std::string v = validate(A, "A");
  if (!v.empty()) return fail(AMG_HIP_EINVAL, v);
  CoarseOnDev C;
  if ((st = upload_coarse(A, -1, &C, false)) != AMG_HIP_OK) return st;  // bit-exact forms only
  if (halfbw) *halfbw = C.w;
  DevMem df, dy, dx;
  HIP_TRY(upload(df, f, (size_t)n));
  HIP_TRY(dy.alloc(sizeof(double) * n));
  HIP_TRY(dx.alloc(sizeof(double) * n));
  HIP_TRY(launch_coarse(C, df.as<double>(), dy.as<double>(), dx.as<double>(), nullptr));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(x, dx.p, sizeof(double) * n, hipMemcpyDeviceToHost));
  return AMG_HIP_OK;
}

amg_hip_status amg_hip_coarse_solve_fast(int64_t n, const int32_t* colptr, const int32_t* rowind,
                                         const double* val, const double* f, double* x,
                                         int64_t* halfbw, int32_t* partition_rows) {
  amg_hip_status st = need_device();
  if (st != AMG_HIP_OK) return st;
  if (n <= 0 || !colptr || !rowind || !val || !f || !x) return fail(AMG_HIP_EINVAL, "bad argument");
  Sparse A = from_raw(n, n, colptr, rowind, val);
  std::string v = validate(A, "A");
  if (!v.empty()) return fail(AMG_HIP_EINVAL, v);
  BandFactor F;
  std::string e = band_factor(A, (size_t)8 << 30, &F);
  if (!e.empty()) return fail(AMG_HIP_EINVAL, e);
  if (halfbw) *halfbw = F.w;
  SpikeFactor SF;
  e = spike_factor(F, &SF);
  if (!e.empty()) return fail(AMG_HIP_EUNSUPPORTED, e);
  if (partition_rows) *partition_rows = SF.c;
  SpikeOnDev D;
  DevMem df, dx;
  HIP_TRY(upload_spike(SF, &D));
  HIP_TRY(upload(df, f, (size_t)n));
  HIP_TRY(dx.alloc(sizeof(double) * n));
  SpikeArgs a = D.a;
  a.f = df.as<double>();
  a.x = dx.as<double>();
  HIP_TRY(launch_spike_solve(a, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(x, dx.p, sizeof(double) * n, hipMemcpyDeviceToHost));
  return AMG_HIP_OK;
}

// SmootherBase::smooth for the built-in kinds, on host arrays.
amg_hip_status amg_hip_smooth(int32_t kind, int64_t n, const int32_t* colptr,
                              const int32_t* rowind, const double* val, double* u,
                              const double* b, double omega, double tol, int64_t every,
                              int64_t n_iters, int64_t* iters, int32_t* converged) {
  amg_hip_status st = need_device();
  if (st != AMG_HIP_OK) return st;
  if (n <= 0 || !colptr || !rowind || !val || !u || !b) return fail(AMG_HIP_EINVAL, "bad argument");
  if (kind == AMG_HIP_SM_SOR && (omega > 2 || omega < 0))
    return fail(AMG_HIP_EINVAL, "`omega` must be in [0, 2] but got omega=" + std::to_string(omega) + "\n");
  if (kind == AMG_HIP_SM_REF_JACOBI && every == 0)
    return fail(AMG_HIP_EINVAL, "AMG::Jacobi divides by compute_error_every_n_iters (smoother.hpp:258); it must be non-zero");
  if (kind == AMG_HIP_SM_SOR && every == 0)
    return fail(AMG_HIP_EINVAL, "AMG::SuccessiveOverRelaxation divides by compute_error_every_n_iters (smoother.hpp:367); it must be non-zero");
  Sparse A = from_raw(n, n, colptr, rowind, val);
  std::string v = validate(A, "A");
  if (!v.empty()) return fail(AMG_HIP_EINVAL, v);
  Sparse Ar = transpose(A);
  DevMat Drows;  // rows of A: rss
  DevMat Dcols;  // CSC arrays as rows: true Jacobi
  const bool sym = same_arrays(A, Ar);
  HIP_TRY(upload_mat(Ar, g_default_layout, &Drows));
  if (!sym) HIP_TRY(upload_mat(A, g_default_layout, &Dcols));
  const DevMat& Dc = sym ? Drows : Dcols;
  DevMem du, db, dt, sc;
  HIP_TRY(upload(du, u, (size_t)n));
  HIP_TRY(upload(db, b, (size_t)n));
  HIP_TRY(dt.alloc(sizeof(double) * n));
  HIP_TRY(sc.alloc(sizeof(double) * 1100));
  LexOnDev Lf, Lb;
  if (kind == AMG_HIP_SM_SPGS) {
    LexSchedule F, B;
    std::string e = build_lex_schedule(A, false, 64, &F);
    if (e.empty()) e = build_lex_schedule(A, true, 64, &B);
    if (!e.empty()) return fail(AMG_HIP_EUNSUPPORTED, e);
    HIP_TRY(upload_lex(F, &Lf));
    HIP_TRY(upload_lex(B, &Lb));
  } else if (kind == AMG_HIP_SM_REF_JACOBI || kind == AMG_HIP_SM_SOR) {
    LexSchedule F;
    std::string e = build_lex_schedule(Ar, false, 64, &F);
    if (!e.empty()) return fail(AMG_HIP_EUNSUPPORTED, e);
    HIP_TRY(upload_lex(F, &Lf));
  } else if (kind == AMG_HIP_SM_JACOBI) {
  } else {
    return fail(AMG_HIP_EUNSUPPORTED, "smoother kind not available as a stand-alone call");
  }
  int64_t iter = 0;
  double error = 100;  // smoother.hpp:194
  double* cur = du.as<double>();
  double* alt = dt.as<double>();
  const bool check = (kind <= AMG_HIP_SM_SOR);
  while (iter < n_iters && (!check || error > tol)) {
    if (kind == AMG_HIP_SM_SPGS) {
      HIP_TRY(launch_gs_lex(Lf.d, db.as<double>(), cur, 0, 1.0, nullptr));
      HIP_TRY(launch_gs_lex(Lb.d, db.as<double>(), cur, 0, 1.0, nullptr));
    } else if (kind == AMG_HIP_SM_REF_JACOBI) {
      HIP_TRY(launch_gs_lex(Lf.d, db.as<double>(), cur, 1, 1.0, nullptr));
    } else if (kind == AMG_HIP_SM_SOR) {
      HIP_TRY(launch_gs_lex(Lf.d, db.as<double>(), cur, 2, omega, nullptr));
    } else {
      HIP_TRY(launch_mat(CSR_JACOBI, Dc, cur, db.as<double>(), alt, omega, nullptr));
      std::swap(cur, alt);
    }
    iter += 1;
    if (check && every != 0 && iter % every == 0) {
      HIP_TRY(launch_mat(CSR_RSSQ, Drows, cur, db.as<double>(), alt, 1.0, nullptr));
      HIP_TRY(launch_sum(n, alt, sc.as<double>() + 1024, sc.as<double>(), 0, nullptr));
      HIP_TRY(hipDeviceSynchronize());
      HIP_TRY(hipMemcpy(&error, sc.as<double>() + 1024, sizeof(double), hipMemcpyDeviceToHost));
    }
  }
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(u, cur, sizeof(double) * n, hipMemcpyDeviceToHost));
  if (iters) *iters = iter;
  if (converged) *converged = error <= tol;
  return AMG_HIP_OK;
}

amg_hip_status amg_hip_smooth_chebyshev(int64_t n, const int32_t* colptr, const int32_t* rowind,
                                        const double* val, double* u, const double* b, int32_t degree,
                                        double lower, double upper, int64_t n_iters) {
  if (n <= 0 || !colptr || !rowind || !val || !u || !b) return fail(AMG_HIP_EINVAL, "bad argument");
  std::string v = cheb_options_error(degree, lower, upper);
  if (!v.empty()) return fail(AMG_HIP_EINVAL, v);
  if (n_iters < 0) return fail(AMG_HIP_EINVAL, "`n_iters` must be >= 0");
  Sparse A = from_raw(n, n, colptr, rowind, val);
  v = validate(A, "A");
  if (!v.empty()) return fail(AMG_HIP_EINVAL, v);
  Sparse Ar = transpose(A);  // the polynomial is in D^-1 A: rows of A
  int64_t zr = -1;
  const double G = gershgorin_host(Ar, &zr);
  if (zr >= 0) return fail(AMG_HIP_EINVAL, cheb_zero_diag(0, zr));
  amg_hip_status st = need_device();
  if (st != AMG_HIP_OK) return st;
  std::vector<double> alpha, beta;
  cheb_coefs(lower * G, upper * G, degree, &alpha, &beta);
  DevMat D;
  HIP_TRY(upload_mat(Ar, g_default_layout, &D));
  DevMem du, db, dt, dd;
  HIP_TRY(upload(du, u, (size_t)n));
  HIP_TRY(upload(db, b, (size_t)n));
  HIP_TRY(dt.alloc(sizeof(double) * n));
  HIP_TRY(dd.alloc(sizeof(double) * n));
  double* cur = du.as<double>();
  double* alt = dt.as<double>();
  for (int64_t it = 0; it < n_iters; ++it)
    for (int j = 0; j < degree; ++j) {
      ChebStep c;
      c.d = dd.as<double>();
      c.alpha = alpha[(size_t)j];
      c.beta = beta[(size_t)j];
      c.first = j == 0;
      c.last = j == degree - 1;
      HIP_TRY(launch_mat_cheb(D, cur, db.as<double>(), alt, c, nullptr));
      std::swap(cur, alt);
    }
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(u, cur, sizeof(double) * n, hipMemcpyDeviceToHost));
  return AMG_HIP_OK;
}

amg_hip_status amg_hip_smooth_line(int64_t n, const int32_t* colptr, const int32_t* rowind, const double* val,
                                   int64_t stride, double omega, int64_t iters, double* u, const double* f) {
  if (n <= 0 || !colptr || !rowind || !val || !u || !f) return fail(AMG_HIP_EINVAL, "bad argument");
  if (stride < 0) return fail(AMG_HIP_EINVAL, "`stride` must be >= 0 (0: the automatic rule)");
  if (iters < 0) return fail(AMG_HIP_EINVAL, "`iters` must be >= 0");
  std::string v = line_options_error(omega);
  if (!v.empty()) return fail(AMG_HIP_EINVAL, v);
  Sparse A = from_raw(n, n, colptr, rowind, val);
  v = validate(A, "A");
  if (!v.empty()) return fail(AMG_HIP_EINVAL, v);
  if (n >= ((int64_t)1 << 31)) return fail(AMG_HIP_EUNSUPPORTED, "line smoother: 2^31 rows or more");
  Sparse Ar = transpose(A);  // T and the residual are taken from the rows of A
  amg_hip_status st = need_device();
  if (st != AMG_HIP_OK) return st;
  DevCsr rows;
  HIP_TRY(upload_csr(Ar, &rows));
  LineOnDev D;
  st = line_setup_dev(0, n, rows.rowptr(), rows.col(), rows.v(), stride, &D);
  if (st != AMG_HIP_OK) return st;
  DevMat M;
  HIP_TRY(upload_mat(Ar, g_default_layout, &M));
  DevMem du, df, dr;
  HIP_TRY(upload(du, u, (size_t)n));
  HIP_TRY(upload(df, f, (size_t)n));
  HIP_TRY(dr.alloc(sizeof(double) * n));
  for (int64_t it = 0; it < iters; ++it)
    HIP_TRY(launch_line_sweep(M, D, du.as<double>(), df.as<double>(), dr.as<double>(), omega, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(u, du.p, sizeof(double) * n, hipMemcpyDeviceToHost));
  return AMG_HIP_OK;
}

static amg_hip_status smooth_line_alt(const std::string& who, int64_t n, const int32_t* colptr, const int32_t* rowind,
                                      const double* val, int32_t dim, const int64_t* dims, int32_t periodic_axes,
                                      double omega, int64_t iters, int32_t reverse, double* u, const double* f) {
  if (n <= 0 || !colptr || !rowind || !val || !u || !f) return fail(AMG_HIP_EINVAL, "bad argument");
  std::string v = tensor_dims_error(dim, dims);
  if (!v.empty()) return fail(AMG_HIP_EINVAL, who + v);
  v = periodic_axes_error(dim, periodic_axes);
  if (!v.empty()) return fail(AMG_HIP_EINVAL, who + v);
  v = grid_size_error(n, dims, true);
  if (!v.empty()) return fail(AMG_HIP_EINVAL, who + v);
  if (iters < 0) return fail(AMG_HIP_EINVAL, "`iters` must be >= 0");
  v = line_options_error(omega);
  if (!v.empty()) return fail(AMG_HIP_EINVAL, v);
  Sparse A = from_raw(n, n, colptr, rowind, val);
  v = validate(A, "A");
  if (!v.empty()) return fail(AMG_HIP_EINVAL, v);
  Sparse Ar = transpose(A);  // T and the residual are taken from the rows of A
  AltOnDev D;
  D.set_grid(n, dims, (uint32_t)periodic_axes);
  amg_hip_status st = alt_setup_host(0, Ar.ptr.data(), Ar.idx.data(), Ar.val.data(), &D);  // before the device
  if (st != AMG_HIP_OK) return st;
  st = need_device();
  if (st != AMG_HIP_OK) return st;
  DevCsr rows;
  HIP_TRY(upload_csr(Ar, &rows));
  st = alt_setup_dev(0, rows.rowptr(), rows.col(), rows.v(), &D);
  if (st != AMG_HIP_OK) return st;
  DevMat M;
  HIP_TRY(upload_mat(Ar, g_default_layout, &M));
  DevMem du, df, dr;
  HIP_TRY(upload(du, u, (size_t)n));
  HIP_TRY(upload(df, f, (size_t)n));
  HIP_TRY(dr.alloc(sizeof(double) * n));
  st = line_subsweeps(iters, line_dirs(AMG_HIP_SM_LINE_ALT, D), reverse != 0, [&](int d) {
    HIP_TRY(launch_alt_subsweep(M, D, d, du.as<double>(), df.as<double>(), dr.as<double>(), omega, nullptr));
    return AMG_HIP_OK;
  });
  if (st != AMG_HIP_OK) return st;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(u, du.p, sizeof(double) * n, hipMemcpyDeviceToHost));
  return AMG_HIP_OK;
}

amg_hip_status amg_hip_smooth_line_alt(int64_t n, const int32_t* colptr, const int32_t* rowind, const double* val,
                                       int32_t dim, const int64_t* dims, double omega, int64_t iters,
                                       int32_t reverse, double* u, const double* f) {
  return smooth_line_alt("amg_hip_smooth_line_alt: ", n, colptr, rowind, val, dim, dims, 0, omega, iters, reverse, u,
                         f);
}
amg_hip_status amg_hip_smooth_line_alt_per(int64_t n, const int32_t* colptr, const int32_t* rowind, const double* val,
                                           int32_t dim, const int64_t* dims, int32_t periodic_axes, double omega,
                                           int64_t iters, int32_t reverse, double* u, const double* f) {
  return smooth_line_alt("amg_hip_smooth_line_alt_per: ", n, colptr, rowind, val, dim, dims, periodic_axes, omega,
                         iters, reverse, u, f);
}

amg_hip_status amg_hip_spgs_sweep(int32_t dir, int64_t n, const int32_t* colptr,
                                  const int32_t* rowind, const double* val, double* u,
                                  const double* b) {
  amg_hip_status st = need_device();
  if (st != AMG_HIP_OK) return st;
  if (n <= 0 || !colptr || !rowind || !val || !u || !b) return fail(AMG_HIP_EINVAL, "bad argument");
  Sparse A = from_raw(n, n, colptr, rowind, val);
  std::string v = validate(A, "A");
  if (!v.empty()) return fail(AMG_HIP_EINVAL, v);
  LexSchedule S;
  std::string e = build_lex_schedule(A, dir < 0, 64, &S);
  if (!e.empty()) return fail(AMG_HIP_EUNSUPPORTED, e);
  LexOnDev L;
  HIP_TRY(upload_lex(S, &L));
  DevMem du, db;
  HIP_TRY(upload(du, u, (size_t)n));
  HIP_TRY(upload(db, b, (size_t)n));
  HIP_TRY(launch_gs_lex(L.d, db.as<double>(), du.as<double>(), 0, 1.0, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(u, du.p, sizeof(double) * n, hipMemcpyDeviceToHost));
  return AMG_HIP_OK;
}

// ---- hipIpc arena + stream-ordered halo exchange ---------------------------------
struct amg_hip_arena_impl {
  void* base = nullptr;
  int64_t bytes = 0;
  int device = 0;
};

amg_hip_status amg_hip_arena_create(int64_t bytes, int32_t device, amg_hip_arena** out) {
  if (!out || bytes <= 0) return fail(AMG_HIP_EINVAL, "bad argument");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(AMG_HIP_EHIP, "no HIP device available (this library has no CPU fallback)");
  if (device < 0) HIP_TRY(hipGetDevice(&device));
  HIP_TRY(hipSetDevice(device));
  std::unique_ptr<amg_hip_arena_impl> a(new amg_hip_arena_impl);
  a->bytes = bytes;
  a->device = device;
  HIP_TRY(hipMalloc(&a->base, (size_t)bytes));
  HIP_TRY(hipMemset(a->base, 0, (size_t)bytes));
  HIP_TRY(hipDeviceSynchronize());
  *out = reinterpret_cast<amg_hip_arena*>(a.release());
  return AMG_HIP_OK;
}
void amg_hip_arena_destroy(amg_hip_arena* h) {
  auto* a = reinterpret_cast<amg_hip_arena_impl*>(h);
  if (!a) return;
  if (a->base) {
    (void)hipSetDevice(a->device);
    (void)hipDeviceSynchronize();
    (void)hipFree(a->base);
  }
  delete a;
}
void* amg_hip_arena_base(const amg_hip_arena* h) {
  return h ? reinterpret_cast<const amg_hip_arena_impl*>(h)->base : nullptr;
}
amg_hip_status amg_hip_arena_export(const amg_hip_arena* h, uint8_t handle[64]) {
  auto* a = reinterpret_cast<const amg_hip_arena_impl*>(h);
  if (!a || !handle) return fail(AMG_HIP_EINVAL, "bad argument");
  static_assert(sizeof(hipIpcMemHandle_t) == 64, "hipIpcMemHandle_t is 64 bytes");
  hipIpcMemHandle_t hd;
  HIP_TRY(hipIpcGetMemHandle(&hd, a->base));
  std::memcpy(handle, &hd, 64);
  return AMG_HIP_OK;
}
amg_hip_status amg_hip_arena_open_peer(const uint8_t handle[64], void** peer_base) {
  if (!handle || !peer_base) return fail(AMG_HIP_EINVAL, "bad argument");
  hipIpcMemHandle_t hd;
  std::memcpy(&hd, handle, 64);
  HIP_TRY(hipIpcOpenMemHandle(peer_base, hd, hipIpcMemLazyEnablePeerAccess));
  return AMG_HIP_OK;
}
amg_hip_status amg_hip_arena_close_peer(void* peer_base) {
  if (!peer_base) return AMG_HIP_OK;
  HIP_TRY(hipIpcCloseMemHandle(peer_base));
  return AMG_HIP_OK;
}

amg_hip_status amg_hip_halo_push_wait(const amg_hip_halo_desc* d, void* stream) {
  if (!d || d->epoch == 0) return fail(AMG_HIP_EINVAL, "bad halo descriptor");
  hipStream_t st = (hipStream_t)stream;
  const uint32_t e = d->epoch;
  const bool to_prev = d->dst_prev && d->bytes_prev > 0, to_next = d->dst_next && d->bytes_next > 0;
  // 1. my previous message on this channel must have been consumed
  if (e > 1) {
    if (to_prev && d->my_ack_from_prev)
      HIP_TRY(hipStreamWaitValue32(st, d->my_ack_from_prev, e - 1, hipStreamWaitValueGte, 0xffffffffu));
    if (to_next && d->my_ack_from_next)
      HIP_TRY(hipStreamWaitValue32(st, d->my_ack_from_next, e - 1, hipStreamWaitValueGte, 0xffffffffu));
  }
  // 2. push + publish
  if (to_prev) {
    HIP_TRY(hipMemcpyAsync(d->dst_prev, d->src_prev, (size_t)d->bytes_prev, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipStreamWriteValue32(st, d->data_flag_at_prev, e, 0));
  }
  if (to_next) {
    HIP_TRY(hipMemcpyAsync(d->dst_next, d->src_next, (size_t)d->bytes_next, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipStreamWriteValue32(st, d->data_flag_at_next, e, 0));
  }
  // 3. wait for the neighbours' data of this epoch
  if (d->recv_from_prev)
    HIP_TRY(hipStreamWaitValue32(st, d->my_data_from_prev, e, hipStreamWaitValueGte, 0xffffffffu));
  if (d->recv_from_next)
    HIP_TRY(hipStreamWaitValue32(st, d->my_data_from_next, e, hipStreamWaitValueGte, 0xffffffffu));
  return AMG_HIP_OK;
}

amg_hip_status amg_hip_halo_ack(const amg_hip_halo_desc* d, void* stream) {
  if (!d || d->epoch == 0) return fail(AMG_HIP_EINVAL, "bad halo descriptor");
  hipStream_t st = (hipStream_t)stream;
  if (d->recv_from_prev && d->ack_flag_at_prev)
    HIP_TRY(hipStreamWriteValue32(st, d->ack_flag_at_prev, d->epoch, 0));
  if (d->recv_from_next && d->ack_flag_at_next)
    HIP_TRY(hipStreamWriteValue32(st, d->ack_flag_at_next, d->epoch, 0));
  return AMG_HIP_OK;
}

amg_hip_status amg_hip_halo_exchange_kernel(const amg_hip_halo_kdesc* d, void* stream) {
  if (!d || !d->timeout) return fail(AMG_HIP_EINVAL, "bad halo descriptor");
  static_assert(sizeof(amg_hip_halo_kdesc) == sizeof(HaloArgs), "layout");
  HaloArgs a;
  std::memcpy(&a, d, sizeof(a));
  HIP_TRY(launch_halo_exchange(a, (hipStream_t)stream));
  return AMG_HIP_OK;
}
amg_hip_status amg_hip_halo_ack_kernel(uint32_t* free_at_prev, uint32_t* free_at_next,
                                       void* stream) {
  HIP_TRY(launch_halo_ack(free_at_prev, free_at_next, (hipStream_t)stream));
  return AMG_HIP_OK;
}
amg_hip_status amg_hip_gather_kernel(const amg_hip_gather_kdesc* d, void* stream) {
  if (!d || d->world < 1 || d->world > GATHER_MAX_RANKS) return fail(AMG_HIP_EINVAL, "bad gather descriptor");
  static_assert(sizeof(amg_hip_gather_kdesc) == sizeof(GatherArgs), "layout");
  GatherArgs a;
  std::memcpy(&a, d, sizeof(a));
  HIP_TRY(launch_gather(a, (hipStream_t)stream));
  return AMG_HIP_OK;
}
amg_hip_status amg_hip_gather_ack_kernel(const amg_hip_gather_kdesc* d, void* stream) {
  if (!d || d->world < 1 || d->world > GATHER_MAX_RANKS) return fail(AMG_HIP_EINVAL, "bad gather descriptor");
  GatherArgs a;
  std::memcpy(&a, d, sizeof(a));
  HIP_TRY(launch_gather_ack(a, (hipStream_t)stream));
  return AMG_HIP_OK;
}
amg_hip_status amg_hip_fill_u32(uint32_t* dev_ptr, int64_t count, uint32_t value, void* stream) {
  if (!dev_ptr || count < 0) return fail(AMG_HIP_EINVAL, "bad argument");
  HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)dev_ptr, (int)value, (size_t)count, (hipStream_t)stream));
  return AMG_HIP_OK;
}

amg_hip_status amg_hip_capture_begin(void* stream) {
  HIP_TRY(hipStreamBeginCapture((hipStream_t)stream, hipStreamCaptureModeRelaxed));
  return AMG_HIP_OK;
}
amg_hip_status amg_hip_capture_end(void* stream, void** graph_exec) {
  if (!graph_exec) return fail(AMG_HIP_EINVAL, "bad argument");
  hipGraph_t g = nullptr;
  HIP_TRY(hipStreamEndCapture((hipStream_t)stream, &g));
  hipGraphExec_t ex = nullptr;
  hipError_t e = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
  (void)hipGraphDestroy(g);
  if (e != hipSuccess) return fail(AMG_HIP_EHIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(e));
  *graph_exec = ex;
  return AMG_HIP_OK;
}
amg_hip_status amg_hip_graph_launch(void* graph_exec, void* stream) {
  if (!graph_exec) return fail(AMG_HIP_EINVAL, "bad argument");
  HIP_TRY(hipGraphLaunch((hipGraphExec_t)graph_exec, (hipStream_t)stream));
  return AMG_HIP_OK;
}
void amg_hip_graph_destroy(void* graph_exec) {
  if (graph_exec) (void)hipGraphExecDestroy((hipGraphExec_t)graph_exec);
}

// ---- generators -----------------------------------------------------------------
int64_t amg_hip_laplacian(int32_t dim, int64_t n, int32_t* colptr, int32_t* rowind,
                          double* val) {
  if ((dim != 2 && dim != 3) || n <= 0) {
    g_err = "laplacian: dim must be 2 or 3 and n positive";
    return -1;
  }
  const double N = std::pow((double)n, dim);
  if (N * (2 * dim + 1) >= 2147483647.0) {
    g_err = "laplacian: nnz exceeds int32 indices";
    return -1;
  }
  if (!colptr && !rowind && !val) {  // size query
    const int64_t nn = (dim == 2) ? n * n : n * n * n;
    const int64_t faces = (dim == 2) ? 2 * n * (n - 1) : 3 * n * n * (n - 1);
    return nn + 2 * faces;
  }
  Sparse A = laplacian(dim, n);
  if (colptr) std::memcpy(colptr, A.ptr.data(), sizeof(int32_t) * A.ptr.size());
  if (rowind) std::memcpy(rowind, A.idx.data(), sizeof(int32_t) * A.idx.size());
  if (val) std::memcpy(val, A.val.data(), sizeof(double) * A.val.size());
  return A.nnz();
}
amg_hip_status amg_hip_rhs(int32_t dim, int64_t n, double* b) {
  if ((dim != 2 && dim != 3) || n <= 0 || !b) return fail(AMG_HIP_EINVAL, "bad argument");
  rhs(dim, n, b);
  return AMG_HIP_OK;
}

// ---- device-pointer launchers ------------------------------------------------------
static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static amg_hip_status dev_csr(int mode, int64_t nrows, int64_t nnz, int32_t max_block_nnz,
                              int32_t max_row_nnz, const int32_t* rowptr, const int32_t* col,
                              const double* val, const double* x, const double* f, double* out,
                              double omega, int64_t diag_shift, void* stream) {
  if (nrows < 0 || nnz < 0 || !rowptr || !col || !val || !x || !out)
    return fail(AMG_HIP_EINVAL, "bad argument");
  if (!aligned16(col) || !aligned16(val))
    return fail(AMG_HIP_EINVAL, "col/val device pointers must be 16-byte aligned");
  if (nrows == 0) return AMG_HIP_OK;
  HIP_TRY(launch_csr(mode, nrows, nnz, max_block_nnz, max_row_nnz, rowptr, col, val, x, f, out,
                     omega, diag_shift, (hipStream_t)stream));
  return AMG_HIP_OK;
}

amg_hip_status amg_hip_dict_probe(int64_t nrows, int64_t ncols, const int32_t* rowptr,
                                  const int32_t* col, const double* val, int64_t diag_shift,
                                  int32_t* n_pairs, int32_t* n_row_types, int32_t* words) {
  if (nrows < 0 || ncols < 0 || !rowptr || (rowptr[nrows] > 0 && (!col || !val)))
    return fail(AMG_HIP_EINVAL, "bad argument");
  Sparse M = from_raw(nrows, ncols, rowptr, col, val);
  std::string v = validate(M, "matrix");
  if (!v.empty()) return fail(AMG_HIP_EINVAL, v);
  DictMat T;
  if (!to_dict(M, diag_shift, &T))
    return fail(AMG_HIP_EUNSUPPORTED, "the matrix does not qualify for the dictionary coding");
  // decode: row type -> code words -> (offset, value) pairs, compare with the input
  const bool typed = !T.rtype.empty();
  for (int64_t r = 0; r < nrows; ++r) {
    uint64_t w[2] = {~(uint64_t)0, ~(uint64_t)0};
    for (int k = 0; k < T.words; ++k)
      w[k] = typed ? T.rwords[(size_t)T.rtype[r] * T.words + k] : T.codes[(size_t)r * T.words + k];
    if (typed)
      for (int k = 0; k < T.words; ++k)
        if (w[k] != T.codes[(size_t)r * T.words + k])
          return fail(AMG_HIP_EHIP, "row type table does not reproduce the code words");
    int j = 0;
    for (int32_t q = rowptr[r]; q < rowptr[r + 1]; ++q, ++j) {
      const int code = (int)((w[j >> 3] >> (8 * (j & 7))) & 0xFF);
      if (code == 0xFF || code >= (int)T.doff.size() ||
          (int64_t)T.doff[code] + r + diag_shift != (int64_t)col[q] ||
          std::memcmp(&T.dval[code], &val[q], sizeof(double)) != 0)
        return fail(AMG_HIP_EHIP, "dictionary coding does not round-trip");
    }
    for (; j < 8 * T.words; ++j)
      if (((w[j >> 3] >> (8 * (j & 7))) & 0xFF) != 0xFF)
        return fail(AMG_HIP_EHIP, "dictionary coding has entries past the end of a row");
  }
  if (n_pairs) *n_pairs = (int32_t)T.doff.size();
  if (n_row_types) {
    int32_t nt = 0;
    if (typed)
      for (uint8_t t : T.rtype) nt = std::max<int32_t>(nt, (int32_t)t + 1);
    *n_row_types = nt;
  }
  if (words) *words = T.words;
  return AMG_HIP_OK;
}

amg_hip_status amg_hip_csr_shape(int64_t nrows, const int32_t* rowptr_host,
                                 int32_t* max_block_nnz, int32_t* max_row_nnz) {
  if (nrows < 0 || !rowptr_host) return fail(AMG_HIP_EINVAL, "bad argument");
  int mb = 0, mr = 0;
  for (int64_t r = 0; r < nrows; ++r) mr = std::max(mr, rowptr_host[r + 1] - rowptr_host[r]);
  for (int64_t r = 0; r < nrows; r += 256) {
    const int64_t e = std::min<int64_t>(r + 256, nrows);
    mb = std::max(mb, rowptr_host[e] - rowptr_host[r]);
  }
  if (max_block_nnz) *max_block_nnz = mb;
  if (max_row_nnz) *max_row_nnz = mr;
  return AMG_HIP_OK;
}

amg_hip_status amg_hip_dev_residual(int64_t nrows, int64_t nnz, int32_t max_block_nnz,
                                    int32_t max_row_nnz, const int32_t* rowptr,
                                    const int32_t* col, const double* val, const double* u,
                                    const double* f, double* r, void* stream) {
  if (!f) return fail(AMG_HIP_EINVAL, "bad argument");
  return dev_csr(CSR_RESID, nrows, nnz, max_block_nnz, max_row_nnz, rowptr, col, val, u, f, r,
                 1.0, 0, stream);
}
amg_hip_status amg_hip_dev_jacobi(int64_t nrows, int64_t nnz, int32_t max_block_nnz,
                                  int32_t max_row_nnz, const int32_t* rowptr,
                                  const int32_t* col, const double* val, const double* u_in,
                                  const double* b, double* u_out, double omega,
                                  int64_t diag_shift, void* stream) {
  if (!b) return fail(AMG_HIP_EINVAL, "bad argument");
  return dev_csr(CSR_JACOBI, nrows, nnz, max_block_nnz, max_row_nnz, rowptr, col, val, u_in, b,
                 u_out, omega, diag_shift, stream);
}
amg_hip_status amg_hip_dev_spmv(int64_t nrows, int64_t nnz, int32_t max_block_nnz,
                                int32_t max_row_nnz, const int32_t* rowptr, const int32_t* col,
                                const double* val, const double* v, double* out, void* stream) {
  return dev_csr(CSR_SPMV, nrows, nnz, max_block_nnz, max_row_nnz, rowptr, col, val, v, nullptr,
                 out, 1.0, 0, stream);
}
amg_hip_status amg_hip_dev_jacobi_from_zero(int64_t nrows, const double* diag, const double* b,
                                            double* u_out, double omega, void* stream) {
  if (nrows < 0 || !diag || !b || !u_out) return fail(AMG_HIP_EINVAL, "bad argument");
  HIP_TRY(launch_jacobi_from_zero(nrows, diag, b, u_out, omega, (hipStream_t)stream));
  return AMG_HIP_OK;
}
// ---- device matrix object: a local CSR block uploaded in the solver's own layout ----
struct amg_hip_devmat_impl {
  DevMat m;
  int device = 0;
  int64_t diag_shift = 0;  // the relative column indices were built against this
};
amg_hip_status amg_hip_devmat_create(int64_t nrows, int64_t ncols, const int32_t* rowptr,
                                     const int32_t* col, const double* val, int32_t layout,
                                     int64_t diag_shift, int32_t device, amg_hip_devmat** out) {
  if (!out || nrows < 0 || ncols < 0 || !rowptr || (rowptr[nrows] > 0 && (!col || !val)))
    return fail(AMG_HIP_EINVAL, "bad argument");
  amg_hip_status st0 = need_device();
  if (st0 != AMG_HIP_OK) return st0;
  Sparse M = from_raw(nrows, ncols, rowptr, col, val);
  std::string v = validate(M, "local matrix");
  if (!v.empty()) return fail(AMG_HIP_EINVAL, v);
  std::unique_ptr<amg_hip_devmat_impl> d(new amg_hip_devmat_impl);
  if (device < 0) HIP_TRY(hipGetDevice(&device));
  HIP_TRY(hipSetDevice(device));
  d->device = device;
  d->diag_shift = diag_shift;
  HIP_TRY(upload_mat_pruned(M, layout, true, &d->m, diag_shift));
  *out = reinterpret_cast<amg_hip_devmat*>(d.release());
  return AMG_HIP_OK;
}
amg_hip_status amg_hip_devmat_layout(const amg_hip_devmat* h, int32_t* layout,
                                     int64_t* matrix_stream_bytes) {
  auto* d = reinterpret_cast<const amg_hip_devmat_impl*>(h);
  if (!d) return fail(AMG_HIP_EINVAL, "bad argument");
  layout_of(d->m, layout, matrix_stream_bytes);
  return AMG_HIP_OK;
}
void amg_hip_devmat_destroy(amg_hip_devmat* h) {
  auto* d = reinterpret_cast<amg_hip_devmat_impl*>(h);
  if (!d) return;
  (void)hipSetDevice(d->device);
  delete d;
}
amg_hip_status amg_hip_devmat_apply(const amg_hip_devmat* h, int32_t op, const double* x,
                                    const double* f, double* out, double omega,
                                    int64_t diag_shift, void* stream) {
  auto* d = reinterpret_cast<const amg_hip_devmat_impl*>(h);
  if (!d || !x || !out) return fail(AMG_HIP_EINVAL, "bad argument");
  int mode;
  switch (op) {
    case 0: mode = CSR_RESID; break;
    case 1: mode = CSR_JACOBI; break;
    case 2: mode = CSR_SPMV; break;
    default: return fail(AMG_HIP_EINVAL, "unknown operation");
  }
  if (mode != CSR_SPMV && !f) return fail(AMG_HIP_EINVAL, "bad argument");
  // residual / SpMV do not look at the diagonal: they decode the relative column
  // indices against the shift the matrix was created with
  if (mode != CSR_JACOBI) diag_shift = d->diag_shift;
  if (diag_shift != d->diag_shift)
    return fail(AMG_HIP_EINVAL, "diag_shift differs from the one the matrix was created with");
  HIP_TRY(launch_mat(mode, d->m, x, f, out, omega, (hipStream_t)stream, diag_shift));
  return AMG_HIP_OK;
}

amg_hip_status amg_hip_dev_axpy1(int64_t n, const double* x, double* y, void* stream) {
  if (n < 0 || !x || !y) return fail(AMG_HIP_EINVAL, "bad argument");
  HIP_TRY(launch_add_inplace(n, x, y, (hipStream_t)stream));
  return AMG_HIP_OK;
}
amg_hip_status amg_hip_dev_sumsq(int64_t n, const double* r, double* out, double* scratch,
                                 void* stream) {
  if (n < 0 || !r || !out || !scratch) return fail(AMG_HIP_EINVAL, "bad argument");
  HIP_TRY(launch_sum(n, r, out, scratch, 1, (hipStream_t)stream));
  return AMG_HIP_OK;
}

// ---- block (multi-right-hand-side) cycles ------------------------------------------
amg_hip_status amg_hip_block_vcycles(amg_hip_solver* s, int32_t k, const double* F, double* U, int32_t n_cycles) {
  if (!s || !F || !U) return fail(AMG_HIP_EINVAL, "null argument");
  if (k < 1 || k > BLOCK_K_MAX) return fail(AMG_HIP_EINVAL, "k must be in 1 .. 16, got " + std::to_string(k));
  if (n_cycles < 0) return fail(AMG_HIP_EINVAL, "n_cycles must be >= 0");
  if (misaligned(F) || misaligned(U)) return fail(AMG_HIP_EINVAL, "F and U must be 16-byte aligned");
  amg_hip_status r = block_supported(s);
  if (r != AMG_HIP_OK) return r;
  if (n_cycles == 0) return AMG_HIP_OK;
  const int kp = block_kp(k);
  if ((r = ensure_block(s, kp)) != AMG_HIP_OK) return r;
  BlockLevel& Q = s->blk.lv[0];
  const int64_t n = s->lv[0].n;
  HIP_TRY(launch_block_pitch(n, k, kp, F, Q.F.as<double>(), true, s->stream));
  HIP_TRY(launch_block_pitch(n, k, kp, U, Q.U.as<double>(), true, s->stream));
  if ((r = run_block_cycles(s, kp, n_cycles)) != AMG_HIP_OK) return r;
  HIP_TRY(launch_block_pitch(n, k, kp, Q.U.as<double>(), U, false, s->stream));
  return AMG_HIP_OK;
}

amg_hip_status amg_hip_block_rss(amg_hip_solver* s, int32_t k, const double* F, const double* U, double* out) {
  if (!s || !F || !U || !out) return fail(AMG_HIP_EINVAL, "null argument");
  if (k < 1 || k > BLOCK_K_MAX) return fail(AMG_HIP_EINVAL, "k must be in 1 .. 16, got " + std::to_string(k));
  if (misaligned(F) || misaligned(U)) return fail(AMG_HIP_EINVAL, "F and U must be 16-byte aligned");
  amg_hip_status r = block_supported(s);
  if (r != AMG_HIP_OK) return r;
  const int kp = block_kp(k);
  if ((r = ensure_block(s, kp)) != AMG_HIP_OK) return r;
  BlockLevel& Q = s->blk.lv[0];
  const int64_t n = s->lv[0].n;
  const DevCsr& A = *Q.rows;
  HIP_TRY(launch_block_pitch(n, k, kp, F, Q.F.as<double>(), true, s->stream));
  HIP_TRY(launch_block_pitch(n, k, kp, U, Q.U.as<double>(), true, s->stream));
  HIP_TRY(launch_block_csr(CSR_RSSQ, kp, n, A.rowptr(), A.col(), A.v(), Q.U.as<double>(), Q.F.as<double>(),
                           Q.T.as<double>(), 1.0, s->stream));
  double h[BLOCK_K_MAX];
  if ((r = block_sums_to_host(s, kp, Q.T.as<double>(), nullptr, h)) != AMG_HIP_OK) return r;
  for (int j = 0; j < k; ++j) out[j] = h[j];
  return AMG_HIP_OK;
}

// k independent PCG recurrences (amg_hip_pcg's, step for step) sharing every SpMV and block cycle.
// The block cycle's level-0 panels are the operands of M^-1: F holds r, U receives z.
amg_hip_status amg_hip_block_pcg(amg_hip_solver* s, int32_t k, const double* Bv, double* X, double rtol,
                                 int64_t max_iters, int64_t* iters, double* relres) {
  if (!s || !Bv || !X) return fail(AMG_HIP_EINVAL, "null argument");
  if (k < 1 || k > BLOCK_K_MAX) return fail(AMG_HIP_EINVAL, "k must be in 1 .. 16, got " + std::to_string(k));
  if (misaligned(Bv) || misaligned(X)) return fail(AMG_HIP_EINVAL, "B and X must be 16-byte aligned");
  if (!(rtol >= 0) || max_iters < 0) return fail(AMG_HIP_EINVAL, "bad tolerance / iteration limit");
  amg_hip_status rc = block_supported(s);
  if (rc != AMG_HIP_OK) return rc;
  const int kp = block_kp(k);
  if ((rc = ensure_block(s, kp)) != AMG_HIP_OK) return rc;
  Block& B = s->blk;
  BlockLevel& Q = B.lv[0];
  const int64_t n = s->lv[0].n;
  const size_t bytes = sizeof(double) * (size_t)n * (size_t)kp;
  hipStream_t st = s->stream;
  if (!B.px.p) {  // at the panels' pitch: a later call with a smaller k reuses them
    const size_t pbytes = sizeof(double) * (size_t)n * (size_t)B.kp_alloc;
    HIP_TRY(B.px.alloc(pbytes));
    HIP_TRY(B.pp.alloc(pbytes));
    HIP_TRY(B.pq.alloc(pbytes));
    HIP_TRY(B.pb.alloc(pbytes));
  }
  const DevCsr& A = *Q.rows;
  double* x = B.px.as<double>();
  double* p = B.pp.as<double>();
  double* q = B.pq.as<double>();
  double* b = B.pb.as<double>();
  double* r = Q.F.as<double>();
  double* z = Q.U.as<double>();
  double* d = B.dots.as<double>();
  double* d_rz = d;
  double* d_pq = d + BLOCK_K_MAX;
  double* d_rzn = d + 2 * BLOCK_K_MAX;
  double* part = B.part.as<double>();
  int32_t* act = B.act.as<int32_t>();
  double h[BLOCK_K_MAX], bnorm[BLOCK_K_MAX], rel[BLOCK_K_MAX];
  int64_t it[BLOCK_K_MAX];
  int32_t on[BLOCK_K_MAX];
  HIP_TRY(launch_block_pitch(n, k, kp, Bv, b, true, st));
  HIP_TRY(launch_block_pitch(n, k, kp, X, x, true, st));
  // s->project_mean (K-Center, pcg_run's steps per column): b = centre(b) in the panel, every z centred in
  // the pass that forms r . z, x centred in all columns at the end; a padded column is zero and stays zero
  const bool project = s->project_mean;
  double* d_sum = d + 4 * BLOCK_K_MAX;  // past block_sums_to_host's
  if (project) {
    HIP_TRY(launch_block_sum(kp, n, b, nullptr, d_sum, part, st));
    HIP_TRY(launch_block_center(kp, n, d_sum, b, st));
  }
  if ((rc = block_sums_to_host(s, kp, b, b, h)) != AMG_HIP_OK) return rc;  // b . b
  for (int j = 0; j < kp; ++j) bnorm[j] = std::sqrt(h[j]);
  HIP_TRY(launch_block_csr(CSR_RESID, kp, n, A.rowptr(), A.col(), A.v(), x, b, r, 1.0, st));  // r = b - A x
  if ((rc = block_sums_to_host(s, kp, r, r, h)) != AMG_HIP_OK) return rc;
  int live = 0;
  for (int j = 0; j < kp; ++j) {
    it[j] = 0;
    rel[j] = bnorm[j] > 0 ? std::sqrt(h[j]) / bnorm[j] : std::sqrt(h[j]);
    on[j] = (j < k && !(rel[j] <= rtol || max_iters == 0)) ? 1 : 0;
    live += on[j];
  }
  if (live > 0) {
    HIP_TRY(hipMemcpy(act, on, sizeof(int32_t) * (size_t)kp, hipMemcpyHostToDevice));
    // z = M^-1 r; p = z; rz = r . z
    HIP_TRY(hipMemsetAsync(z, 0, bytes, st));
    if ((rc = run_block_cycles(s, kp, 1)) != AMG_HIP_OK) return rc;
    if (project) {  // z = centre(z) ahead of p = z
      HIP_TRY(launch_block_sum(kp, n, z, nullptr, d_sum, part, st));
      HIP_TRY(launch_block_center_dot(kp, n, d_sum, z, r, d_rz, part, st));
      HIP_TRY(hipMemcpyAsync(p, z, bytes, hipMemcpyDeviceToDevice, st));
    } else {
      HIP_TRY(hipMemcpyAsync(p, z, bytes, hipMemcpyDeviceToDevice, st));
      HIP_TRY(launch_block_sum(kp, n, r, z, d_rz, part, st));
    }
  }
  while (live > 0) {
    HIP_TRY(launch_block_csr(CSR_SPMV, kp, n, A.rowptr(), A.col(), A.v(), p, nullptr, q, 1.0, st));  // q = A p
    HIP_TRY(launch_block_sum(kp, n, p, q, d_pq, part, st));
    HIP_TRY(launch_block_pcg_update_xr(kp, n, d_rz, d_pq, act, x, r, p, q, st));  // alpha = rz / pq
    if ((rc = block_sums_to_host(s, kp, r, r, h)) != AMG_HIP_OK) return rc;
    live = 0;
    for (int j = 0; j < kp; ++j) {
      if (!on[j]) continue;
      it[j] += 1;
      rel[j] = bnorm[j] > 0 ? std::sqrt(h[j]) / bnorm[j] : std::sqrt(h[j]);
      if (!(rel[j] > rtol) || it[j] >= max_iters) on[j] = 0;  // NaN stops too
      live += on[j];
    }
    if (live == 0) break;
    HIP_TRY(hipMemcpy(act, on, sizeof(int32_t) * (size_t)kp, hipMemcpyHostToDevice));
    HIP_TRY(hipMemsetAsync(z, 0, bytes, st));
    if ((rc = run_block_cycles(s, kp, 1)) != AMG_HIP_OK) return rc;  // z = M^-1 r
    if (project) {
      HIP_TRY(launch_block_sum(kp, n, z, nullptr, d_sum, part, st));
      HIP_TRY(launch_block_center_dot(kp, n, d_sum, z, r, d_rzn, part, st));
    } else {
      HIP_TRY(launch_block_sum(kp, n, r, z, d_rzn, part, st));
    }
    HIP_TRY(launch_block_pcg_update_p(kp, n, d_rzn, d_rz, act, p, z, st));  // beta = rz_new / rz
    HIP_TRY(hipMemcpyAsync(d_rz, d_rzn, sizeof(double) * (size_t)kp, hipMemcpyDeviceToDevice, st));
  }
  if (project) {
    HIP_TRY(launch_block_sum(kp, n, x, nullptr, d_sum, part, st));
    HIP_TRY(launch_block_center(kp, n, d_sum, x, st));
  }
  HIP_TRY(launch_block_pitch(n, k, kp, x, X, false, st));
  HIP_TRY(hipStreamSynchronize(st));
  for (int j = 0; j < k; ++j) {
    if (iters) iters[j] = it[j];
    if (relres) relres[j] = rel[j];
  }
  return AMG_HIP_OK;
}

amg_hip_status amg_hip_block_must_move(amg_hip_solver* s, int32_t k, double* bytes) {
  if (!s || !bytes) return fail(AMG_HIP_EINVAL, "null argument");
  if (k < 1 || k > BLOCK_K_MAX) return fail(AMG_HIP_EINVAL, "k must be in 1 .. 16, got " + std::to_string(k));
  amg_hip_status r = block_supported(s);
  if (r != AMG_HIP_OK) return r;
  const int kp = block_kp(k);
  if ((r = ensure_block(s, kp)) != AMG_HIP_OK) return r;
  StepCtx X{s->stream, false};
  if ((r = enqueue_block_vcycle(s, kp, X)) != AMG_HIP_OK) return r;
  *bytes = X.once + (double)k * X.per_col;
  return AMG_HIP_OK;
}

}  // extern "C"
