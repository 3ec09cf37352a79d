// Launchers of the gfx950 kernels (kernels.hip).  Device pointers only.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

namespace amg_hip {

enum CsrMode {
  CSR_RESID = 0,   // out = f - A x   (ascending column order per row)
  CSR_JACOBI = 1,  // out = x_i + omega*((f_i - sum_{j!=i} a_ij x_j)/a_ii - x_i)
  CSR_SPMV = 2,    // out = A x
  CSR_RSSQ = 3,    // out_i = (f_i - (A x)_i)^2
  CSR_GS = 4,      // in-place Gauss-Seidel update of one colour
  CSR_JACOBI_P = 5,// Jacobi sweep whose input is x + P*uH (linear P), K-SELL only
  CSR_SPMV_ADD = 6,// out = f + A x (f may be out: the prolongation-and-add u_h = u_h + P u_H of a
                   // custom interpolator, multigrid.hpp:294-296, in one launch), K-CSR only
  CSR_CHEB = 7     // one Chebyshev step (launch_mat_cheb): t_i as CSR_JACOBI computes it, then
                   //   d_i = alpha d_i + beta (t_i - x_i)  (first step: beta (t_i - x_i), d not read)
                   //   out_i = x_i + d_i                    (last step: d not written)
};
// Template MODE of the kernel a Chebyshev step launches (what rocprofv3 prints): 16 + first + 2 last
constexpr int cheb_kernel_mode(bool first, bool last) { return 16 + (first ? 1 : 0) + (last ? 2 : 0); }
struct ChebStep {
  double* d = nullptr;  // n doubles, 16-byte aligned
  double alpha = 0.0, beta = 0.0;
  bool first = true, last = true;
};

// one workgroup runs the whole symmetric pass over all colours (small levels); starts_dev:
// nc + 1 storage-row offsets on the device
hipError_t launch_dict_gs_sweep(int nc, const int32_t* starts_dev, int64_t n_storage, int words, int wmax,
                                const uint64_t* codes, const int32_t* rowid, const int32_t* doff,
                                const double* dval, int ntab, const double* f, double* u,
                                hipStream_t st);
// max_block_nnz: max entries in any 256-row block; max_row_nnz: longest row.
hipError_t launch_csr(int mode, int64_t n, int64_t nnz, int max_block_nnz,
                      int max_row_nnz, const int32_t* rowptr, const int32_t* col,
                      const double* val, const double* x, const double* f,
                      double* out, double omega, int64_t diag_shift, hipStream_t st);
// CSR_CHEB on the three layouts: same row walk and division as CSR_JACOBI (bit-identical results
// across layouts); a first step is bit for bit the CSR_JACOBI sweep with omega = beta.
hipError_t launch_csr_cheb(int64_t n, int64_t nnz, int max_block_nnz, int max_row_nnz, const int32_t* rowptr,
                           const int32_t* col, const double* val, const double* x, const double* f, double* out,
                           const ChebStep& c, hipStream_t st);
hipError_t launch_sell_cheb(int64_t n, int idx16, const int64_t* soff, const void* scol, const double* sval,
                            const double* x, const double* f, double* out, const ChebStep& c, hipStream_t st);
// Gershgorin bound of D^-1 A on a device CSR matrix: out[0] = bits of max_i (sum_j |a_ij|) / |a_ii|
// (row sums in ascending column order, the host's order), out[1] = smallest row whose diagonal is
// zero or absent.  out: 2 words, set by the launcher (stream-ordered) to {0, ~0}.
hipError_t launch_gershgorin(int64_t n, const int32_t* rowptr, const int32_t* col, const double* val,
                             uint64_t* out, hipStream_t st);
// K-Line, the line-relaxation smoother (AMG_HIP_SM_LINE_JACOBI): T = the entries of A at column
// offsets 0, +s, -s, a tridiagonal matrix on each of the min(s, n) chains of rows c, c + s, ...
// Every chain is cut with period LINE_SEG (31 interior rows, one separator); the arrays hold the
// factors of the interior blocks, of the separators' Schur complement, and the two spike vectors
// (kernels.hip: K-Line).  n doubles each, 1 <= s <= n < 2^31 (the launchers refuse anything else; s = n
// stands for every stride >= n: each row its own chain).
constexpr int LINE_SEG = 32;
// T = double: the cycle and the set-up.  T = float: the single-precision cycle's float copies of the
// same factors (no float elimination); the set-up-only members stay at their defaults there.
template <typename T>
struct LineRefT {
  int64_t n = 0, s = 1;
  int64_t m = 0;  // set-up only, > 0: chain positions come in grid lines of m; entries across a line end stay out of T
  int32_t cyc = 0;  // set-up only, with m >= 3: 1 = T' of a cyclic line (SeamRef), 2 = its transpose
  T *dl = nullptr, *ip = nullptr, *cp = nullptr, *v = nullptr, *w = nullptr;
};
using LineRef = LineRefT<double>;
// stride rule on a device CSR matrix: out[1] = the largest distance d = |j - i| >= 1 whose weight
// w(d) = sum |a_ij| reaches (1 - 1e-9) max w, or 1 without off-diagonal entries; out[0] = bits of
// max w.  wd: n doubles of scratch.  line_stride_host: the same rule on host arrays.
hipError_t launch_line_stride(int64_t n, const int32_t* rowptr, const int32_t* col, const double* val, double* wd,
                              uint64_t* out, hipStream_t st);
int64_t line_stride_host(int64_t n, const int32_t* rowptr, const int32_t* col, const double* val);
// extract T from CSR(A) and factor it into L's arrays; bad[0] = smallest row whose pivot is zero or
// not finite, else ~0 (bad: 2 words).  line_setup_host: the same elimination on the host, factors
// discarded; returns that row or -1.
hipError_t launch_line_setup(const LineRef& L, const int32_t* rowptr, const int32_t* col, const double* val,
                             uint64_t* bad, hipStream_t st);
int64_t line_setup_host(int64_t n, int64_t s, const int32_t* rowptr, const int32_t* col, const double* val,
                        int64_t m = 0, int cyc = 0);
// u += omega T^-1 r.  y: n doubles of scratch, r is not written.  Three launches (two on a level
// without separators): line_seg_kernel, line_sep_few_kernel or line_sep_many_kernel, line_update_kernel.
hipError_t launch_line_solve(const LineRef& L, const double* r, double* y, double* u, double omega,
                             hipStream_t st);
bool line_few_chains(int64_t s);  // the reduced systems run as one workgroup per chain
// The solve in float (single-precision cycle): the same kernels instantiated on float.  y: n floats of scratch.
hipError_t launch_line_solve_f32(const LineRefT<float>& L, const float* r, float* y, float* u, float omega,
                                 hipStream_t st);
// K-LineX, the x lines of a tensor grid (AMG_HIP_SM_LINE_ALT): n / nx lines of nx rows, each
// contiguous in memory.  T_x = the diagonal of A and its entries at column offsets +-1 that stay
// inside a line; dl, ip, cp (n doubles each) are its plain Thomas factors, dl = 0 on the first and
// cp = 0 on the last row of every line.  A wave walks LINEX_RUNS runs of whole lines (linex_run(nx)
// rows each) in chunks of LINEX_COLS columns through LDS (kernels.hip: K-LineX).  n < 2^31.
constexpr int LINEX_COLS = 64, LINEX_RUNS = 8;
template <typename T>
struct LineXRefT {
  int64_t n = 0, nx = 1;
  T *dl = nullptr, *ip = nullptr, *cp = nullptr;
  int32_t cyc = 0;  // set-up only, with nx >= 3: as LineRef::cyc
};
using LineXRef = LineXRefT<double>;
int64_t linex_run(int64_t nx);  // rows of one run: nx, or the whole lines that fit LINEX_COLS
// extract T_x from CSR(A) and factor it; bad as launch_line_setup.  linex_setup_host: the same
// elimination on the host, factors discarded; returns the first row with a bad pivot or -1.
hipError_t launch_linex_setup(const LineXRef& L, const int32_t* rowptr, const int32_t* col, const double* val,
                              uint64_t* bad, hipStream_t st);
int64_t linex_setup_host(int64_t n, int64_t nx, const int32_t* rowptr, const int32_t* col, const double* val,
                         int cyc = 0);
// u += omega T_x^-1 r; r is overwritten (the forward values).  Two launches.
hipError_t launch_linex_solve(const LineXRef& L, double* r, double* u, double omega, hipStream_t st);
// the same two launches on float copies of dl, ip, cp (chunks of LINEX_COLS columns as in double)
hipError_t launch_linex_solve_f32(const LineXRefT<float>& L, float* r, float* u, float omega, hipStream_t st);
// K-LineSeam, cyclic lines along a periodic axis (AMG_HIP_SM_LINE_ALT with cyclic_lines): the lines of
// stride s and length m >= 3 (n a multiple of s m; row i on position (i / s) % m of its line, first row
// i0, last row i1) carry the wrap entries alpha = a(i0, i1), beta = a(i1, i0).  With gamma = -a(i0, i0),
//   T' = the open T with the diagonal d(i0) - gamma and d(i1) - alpha beta / gamma (LineRef::cyc = 1),
//   u = gamma e(i0) + beta e(i1), v = e(i0) + (alpha / gamma) e(i1):   cyclic T = T' + u v^T,
// so T^-1 r = T'^-1 (r - fac u), fac = (p . r) / den, p = T'^-T v, den = 1 + v . T'^-1 u
// (Sherman-Morrison).  p: n doubles; coef: den | gamma | beta, n / m doubles each.
template <typename T>
struct SeamRefT {
  int64_t n = 0, s = 1, m = 0;
  const T* p = nullptr;
  const T* coef = nullptr;
};
using SeamRef = SeamRefT<double>;
// set-up: u and v (n doubles each); then coef from q = T'^-1 u, bad as launch_line_setup (the first
// row of a line whose den is zero or not finite).  seam_setup_host: the den check on the host with a
// plain Thomas solve; returns that row or -1.
hipError_t launch_seam_rhs(int64_t n, int64_t s, int64_t m, const int32_t* rowptr, const int32_t* col,
                           const double* val, double* u, double* v, hipStream_t st);
hipError_t launch_seam_coef(int64_t n, int64_t s, int64_t m, const int32_t* rowptr, const int32_t* col,
                            const double* val, const double* q, double* coef, uint64_t* bad, hipStream_t st);
int64_t seam_setup_host(int64_t n, int64_t s, int64_t m, const int32_t* rowptr, const int32_t* col,
                        const double* val);
// r(i0) -= fac gamma, r(i1) -= fac beta on every line, in place.  One launch.
hipError_t launch_line_seam(const SeamRef& S, double* r, hipStream_t st);
// the same launch on float copies of p and coef
hipError_t launch_line_seam_f32(const SeamRefT<float>& S, float* r, hipStream_t st);
// Same operations on a SELL-64 matrix (64-row panels, lane-interleaved):
// soff[n/64 + 1] panel offsets, scol/sval padded with col = -1.
// idx16 bit 0: scol holds int16 offsets from the diagonal column (pad -32768);
// bit 1: stream the matrix / f / out with non-temporal accesses
hipError_t launch_sell(int mode, int64_t n, int idx16, const int64_t* soff,
                       const void* scol, const double* sval, const double* x,
                       const double* f, double* out, double omega, int64_t diag_shift,
                       hipStream_t st);
// out = Jacobi sweep applied to (u + P uH), P = LinearInterpolator prolongation:
// prolongation + add (multigrid.hpp:294-296) fused into the first post-smoothing
// sweep; u itself is not modified.
// K-Dict: dictionary-coded rows (host_setup.hpp: DictMat); modes as launch_sell.
struct DictRef {  // device pointers of one dictionary-coded matrix
  int words = 1, wmax = 0, nt = 0, ntab = 0;
  const uint64_t* codes = nullptr;   // n * words code words (unused when rtype is set)
  const uint8_t* rtype = nullptr;    // optional: one byte per row into rwords
  const uint64_t* rwords = nullptr;  // 256 * words, entry 255 = all 0xFF
  const int32_t* doff = nullptr;     // pair table: column offset from the diagonal column
  const double* dval = nullptr;      //             value
  int scan_new = 99;                 // most entries of a row on one side beyond +-1 (K-GS-scan)
  int hb = 0;                        // largest |column offset| (3-D levels: ~ one grid plane): tile order
  // per row type, for waves whose rows all share one 7- / 15-point stencil type (scalar loads): utd =
  // {off-diagonal value or +0.0 [16], value [16], diagonal}, uti = {offset in rows [16], mask of
  // slots in use, pattern 7 / 15 / 0}; null: none
  const double* utd = nullptr;
  const int32_t* uti = nullptr;
};
void set_xcd_mapping(int on);  // contiguous run of tiles per XCD (default on)
void set_dict_rows_per_lane(int r);  // 1 or 2 (default), tuning / test switch
void set_dict_stencil(int on);       // paired-load path for wave-uniform 7- / 15-point rows (default on)
hipError_t launch_dict(int mode, int64_t n, const DictRef& D, const double* x, const double* f,
                       double* out, double omega, int64_t diag_shift, hipStream_t st);
hipError_t launch_dict_cheb(int64_t n, const DictRef& D, const double* x, const double* f, double* out,
                            const ChebStep& c, hipStream_t st);
// mode: a CsrMode, or cheb_kernel_mode(...) for a Chebyshev step
void dict_kernel_name(int mode, int64_t n, const DictRef& D, const void* f, const void* out,
                      char* buf, size_t cap);
// one colour of the multicolour GS sweep on a dictionary-coded colour-permuted copy
hipError_t launch_dict_gs_color(int64_t p0, int64_t count, int words, int wmax,
                                const uint64_t* codes, const int32_t* rowid, const int32_t* doff,
                                const double* dval, int ntab, const double* f, double* u,
                                hipStream_t st);
// fused forms for the true-Jacobi V-cycle on linear-interpolation levels (kernels.hip):
// r = f - A x (written), f_H = R r, and either uH1 = first Jacobi sweep of the coarse level
// from zero (needs diagH) or, with uH1 == nullptr, uH0 = 0
hipError_t launch_dict_resid_restrict(int64_t n, const DictRef& D, const double* x,
                                      const double* f, double* r_out, int64_t nH, double* fH,
                                      const double* diagH, double* uH1, double* uH0,
                                      double omega, hipStream_t st);
// out = Jacobi sweep of x on this (coarse) level, then uh += P out on the finer level
hipError_t launch_dict_jacobi_prolong(int64_t n, const DictRef& D, const double* x,
                                      const double* f, double* out, double omega, int64_t n_h,
                                      const double* uh_in, double* uh_out, hipStream_t st);
// Two sweeps in one launch on small levels (narrow band, hb = half-bandwidth in rows):
//   down: u_out = Jacobi(a); r = f - A u_out (r_out optional); f_H = R r; uH1 = first coarse sweep
//   up:   t = Jacobi(a) (not stored); u_out = Jacobi(t); uh_out = uh_in + P u_out
bool dict_pair_ok(int64_t n, const DictRef& D, int hb, const void* a, const void* b, const void* c);
hipError_t launch_dict_pair_down(int64_t n, const DictRef& D, int hb, const double* a,
                                 const double* f, double* u_out, double* r_out, int64_t nH,
                                 double* fH, const double* diagH, double* uH1, double omega,
                                 hipStream_t st);
hipError_t launch_dict_pair_up(int64_t n, const DictRef& D, int hb, const double* a,
                               const double* f, double* u_out, double omega, int64_t n_h,
                               const double* uh_in, double* uh_out, hipStream_t st);
// K-Duo: the pair launches of two consecutive pair levels (0 = l, 1 = l+1, 2 = l+2) as one launch.
//   down: launch_dict_pair_down of l (a0 = tmp_l), then of l+1 whose first sweep stays on chip;
//         v2_out = first sweep of level l+2
//   up:   launch_dict_pair_up of l+1 (a1 = tmp_{l+1}), then of l on u0_in + P u_{l+1} formed on chip;
//         the result of level l goes to u0_out (not u0_in: neighbouring tiles read its halo)
// duo_windows_host: the windows of both legs (kernels.hip: the DW_* indices) for tiles of tile_rows
// rows of level l; 0 when all of them are within the kernels' capacities.
constexpr int AMG_DUO_WINDOWS_LEN = 31;
int duo_windows_host(int hb0, int hb1, int tile_rows, int32_t* out);
// rows the tile `tile` owns on levels l, l+1, l+2 as three half-open ranges, before clipping to the
// levels' sizes (the kernels' own function); the tile height the launchers use under half-bandwidth hb0
int duo_owned_host(int tile, int tile_rows, int32_t* out);
int duo_tile_rows(int hb0);
bool dict_duo_ok(int64_t n0, const DictRef& D0, int hb0, int64_t n1, const DictRef& D1, int hb1, int64_t n2);
hipError_t launch_dict_duo_down(int64_t n0, const DictRef& D0, int hb0, int64_t n1, const DictRef& D1, int hb1,
                                const double* a0, const double* f0, double* u0_out, double* r0_out,
                                double* f1_out, const double* diag1, double* u1_out, double* r1_out, int64_t n2,
                                double* f2_out, const double* diag2, double* v2_out, double omega,
                                hipStream_t st);
hipError_t launch_dict_duo_up(int64_t n0, const DictRef& D0, int hb0, int64_t n1, const DictRef& D1, int hb1,
                              const double* a1, const double* f1, double* u1_out, const double* u0_in,
                              const double* f0, double* u0_out, double omega, int64_t n_h, const double* uh_in,
                              double* uh_out, hipStream_t st);
// K-Tail (kernels.hip): the deepest levels of the 2+2 true-Jacobi cycle -- down-legs of levels
// lt .. L-2, the coarsest solve (K-BandChain operands), up-legs and the prolongation into level
// lt - 1 -- in ONE launch of one workgroup.
constexpr int TAIL_LEVELS_MAX = 6;
struct TailLevelRef {
  int n, hbw, words, ntab;
  const uint8_t* rtype;
  const uint64_t* rwords;
  const int32_t* doff;
  const double* dval;
  const double* f;
  double* u;
  double* tmp;
  const double* diag;
};
struct TailRef {
  int nlev;
  TailLevelRef L[TAIL_LEVELS_MAX];
  int nc, wc;
  const double *cf, *cb, *dg;
  double *fc, *uc, *tmpc;
  const double* diagc;
  int n_fine;
  const double* uf_in;
  double* uf_out;
  double omega;
};
bool tail_level_ok(int64_t n, const DictRef& D, int hb);
int tail_max_coarse();
size_t tail_lds_bytes(const TailRef& A);  // LDS the level vectors, tables and the coarsest factor need
size_t tail_lds_capacity();               // ... and what the kernel has (static: 144 KB)
hipError_t launch_tail(const TailRef& A, hipStream_t st);

// K-Patch (kernels.hip): a level's whole down-leg / up-leg of the 2+2 true-Jacobi cycle in
// one launch over 2-D patches of the level (temporal blocking).  ptab: per (row type, slot)
// {off-diagonal value or +0.0, diagonal value or +0.0, value, LDS offset dj * pitch + di or
// -1e9 for an unused slot} as 4 doubles, `un` slots per type (patch_un(longest row)),
// nent = ntypes * un; m = pitch of the band (line length of the flat index).
struct PatchRef {
  const uint8_t* rtype = nullptr;
  const double* ptab = nullptr;
  // the same table per type for the wave-uniform path (scalar loads): utabd = per type
  // {aJ[un], value[un], diagonal}, utabi = per type {LDS offset[un], mask of off-diagonal
  // slots, mask of slots in use}
  const double* utabd = nullptr;
  const int32_t* utabi = nullptr;
  // geometry of the launch: halo rings of lines = dependent stencil stages that run on the loaded
  // data (3: tiles of 42 lines, 2: tiles of 44 lines -- patch_tile_lines).  The tile grid, the
  // instantiation and the meaning of tflag / cflag all follow from it: the flags handed over here
  // must have been built for this very ring count.
  int rings = 3;
  // per tile of the level: the row type every row of the tile and its halo has, or 255
  // (launch_patch_tile_flags); null = always take the general path
  const uint8_t* tflag = nullptr;
  // flag 254 = column-typed tile: every held row inside the matrix, every held column of one row type over
  // all held lines; ctype[tile * patch_frame_columns(rings) + column] is that type.  null: the flags hold no 254
  // (ctype: launch_patch_tile_flags / launch_patch_seam_flags, built beside tflag)
  const uint8_t* ctype = nullptr;
  int nent = 0, ntypes = 0, un = 0, nt = 0;
  int umask = 0;  // slots (3 x 3, bit = slot) of the level's interior row type: selects the kernel kind
  // down-leg: per tile 1 when every coarse row under it has the diagonal dHu (launch_patch_coarse_flags)
  const uint8_t* cflag = nullptr;
  double dHu = 0.0;
};
// (both: for the tiles of a launch with `rings` rings)
hipError_t launch_patch_coarse_flags(int64_t n, int64_t m, int rings, int64_t nH, const double* diagH,
                                     double dref, uint8_t* cflag, hipStream_t st);
// flag == null: only *n_tiles is computed (the size of the array)
hipError_t launch_patch_tile_flags(int64_t n, int64_t m, int rings, const uint8_t* rtype, int ntypes,
                                   uint8_t* flag, int64_t* n_tiles, hipStream_t st, uint8_t* ctype = nullptr);
// columns of the frame a launch of `rings` rings holds (72; the seam's, 5 rings: 76): the pitch of PatchRef::ctype
int patch_frame_columns(int rings);
bool patch_geometry_ok(int64_t n, int64_t m);
int patch_un(int longest_row);
int patch_default_umask(int un);
int patch_kind_umask(int un, int umask);
int patch_lds_pitch();
int patch_max_entries();
// first: both pre-sweeps (x = u) else the second only (x = result of the first sweep);
// u_out = smoothed level vector (never x), r_out optional, f_H / uH1 as launch_dict_resid_restrict.
// uH1 == nullptr: f_H alone is stored (neither diagH nor P.dHu is read): for a coarse level whose
// own down-leg runs with xf.  xf (never with first): x is not read; the kernel forms the first
// sweep from f and the row types' diagonals, bit for bit what uH1 of the finer level would hold.
hipError_t launch_patch_down(bool first, int64_t n, int64_t m, const PatchRef& P, const double* x,
                             const double* f, double* u_out, double* r_out, int64_t nH, double* fH,
                             const double* diagH, double* uH1, double omega, hipStream_t st,
                             int64_t line_lo = 0, int64_t line_hi = -1, bool xf = false);
// The patch launchers take a range of grid lines [line_lo, line_hi) (line_hi < 0: the whole
// level): only the tiles that meet it run (row-block sharding, solver.cpp "slab").
int patch_tile_lines(int rings);  // output lines of a tile: 48 - 2 rings
// rings of a Jacobi leg on tall tiles: 3 for the level-0 down-leg (first: sweep, sweep, residual on
// the loaded data), 2 for every other leg.  launch_patch_down refuses fewer rings than its leg needs.
int patch_leg_rings(bool first);
// u_out = two Jacobi sweeps of (x + P uH); u_out must not be x
hipError_t launch_patch_up(int64_t n, int64_t m, const PatchRef& P, const double* x, const double* f,
                           const double* uH, int64_t nH, double* u_out, double omega,
                           hipStream_t st, int64_t line_lo = 0, int64_t line_hi = -1);
// The level-0 seam between two cycles, one launch: u_out = the two post-sweeps of (x + P uH) followed
// by the two pre-sweeps of the next cycle, fH = the restricted residual of u_out (u_out must not be x).
// Tiles of patch_seam_lines() lines on five halo rings: P.rings == 5 and P.tflag from
// launch_patch_seam_flags (or null).  5-point levels only (patch_un(P.un) == 5).
int patch_seam_lines();
hipError_t launch_patch_seam_flags(int64_t n, int64_t m, const uint8_t* rtype, int ntypes, uint8_t* flag,
                                   int64_t* n_tiles, hipStream_t st, uint8_t* ctype = nullptr);
hipError_t launch_patch_seam(int64_t n, int64_t m, const PatchRef& P, const double* x, const double* f,
                             const double* uH, int64_t nH, double* u_out, double* fH, double omega,
                             hipStream_t st);
// Multicolour Gauss-Seidel on patches: up to patch_rb_max_stages(tail) colour stages per launch
// (stages = patch_rb_stages(colours, count)), u_out != x.  prolong: the input is x + P uH;
// tail: followed by the residual (r_out optional), the restriction into fH and the zeroing of
// uH_zero (optional).  colour(row) = 2-bit entry ((row / m) & 1) * 6 + column class of ctab; column
// classes of c = row % m: 0: c == 0, 1: c == 1, 2: c == m-2, 3: c == m-1, else 4 + (c & 1).
int patch_rb_max_stages(bool tail);
uint32_t patch_rb_stages(const int* colors, int count);
hipError_t launch_patch_rb(bool prolong, bool tail, int64_t n, int64_t m, const PatchRef& P, const double* x,
                           const double* f, const double* uH, int64_t nH, double* u_out, double* r_out,
                           double* fH, double* uH_zero, uint32_t stages, uint32_t ctab, hipStream_t st,
                           int64_t line_lo = 0, int64_t line_hi = -1);
// K-March (kernels.hip): two true-Jacobi sweeps x -> out of a 3-D 7-point level (rows = plane * m *
// lines + line * m + column) in one plane-marching pass.  wtab: per row type 8 doubles {w(-M), w(-m),
// w(-1), w(+1), w(+m), w(+M), diagonal, 0} (+0.0 where the type has no entry); tint / wint / dint: the
// interior type and its values.  out != x.
struct MarchRef {
  int m = 0, lines = 0, planes = 0, ntypes = 0, tint = -1, chunk_planes = 0;
  double omega = 1.0, dint = 0.0;
  double wint[6] = {0, 0, 0, 0, 0, 0};
  const double* wtab = nullptr;
  const uint8_t* rtype = nullptr;
  const double* x = nullptr;
  const double* f = nullptr;
  double* out = nullptr;
};
bool march_ok(const MarchRef& A);
hipError_t launch_march(MarchRef A, hipStream_t st);
// setup: *bad = 1 when a row of type t sits on a box face that forbid.bits[t] rules out
// (1: column 0, 2: column m-1, 4: line 0, 8: line lines-1) or its type is >= ntypes
struct MarchForbid {
  int ntypes = 0;
  uint8_t bits[64] = {};
};
hipError_t launch_march_box_check(int64_t n, int m, int lines, const MarchForbid& F, const uint8_t* rtype,
                                  int32_t* bad, hipStream_t st);
// K-Strip (kernels.hip): the colour stages of a narrow level's whole leg in one launch over strips
// of T rows (+ halo), any colouring (colour byte per row, < 16 colours); stages: 4 bits per stage.
// prolong: the input is x + P uH; tail: followed by the residual (r_out optional), the restriction
// into fH and the zeroing of uH_zero (optional).  u_out != x.  The dictionary must be row-typed.
struct StripRef {
  int n = 0, nH = 0, T = 0, H = 0, hbw = 0, nst = 0, ntab = 0;
  uint64_t stages = 0;
  const uint8_t* rtype = nullptr;
  const uint64_t* rwords = nullptr;
  const int32_t* doff = nullptr;
  const double* dval = nullptr;
  const uint8_t* color = nullptr;
  const double* x = nullptr;
  const double* f = nullptr;
  double* u_out = nullptr;
  double* r_out = nullptr;
  const double* uH = nullptr;
  double* fH = nullptr;
  double* uH_zero = nullptr;
};
int strip_window_max();
hipError_t launch_mc_strip(bool prolong, bool tail, StripRef A, const DictRef& D, hipStream_t st);
// the instantiation that launch runs, as a profiler prints it
void mc_strip_kernel_name(const DictRef& D, bool prolong, bool tail, char* buf, size_t cap);
// uh_out = uh_in + P uH for the linear interpolation pair (16-byte aligned vectors)
hipError_t launch_linear_prolong_to(int64_t n_h, int64_t n_H, const double* uH,
                                    const double* uh_in, double* uh_out, hipStream_t st);
hipError_t launch_sell_jacobi_prolong(int64_t n, int idx16, const int64_t* soff,
                                      const void* scol, const double* sval, const double* u,
                                      const double* uH, int64_t nH, const double* f, double* out,
                                      double omega, hipStream_t st);
// out = Jacobi sweep applied to u == 0: needs only the diagonal and f.
hipError_t launch_jacobi_from_zero(int64_t n, const double* diag, const double* f, double* out,
                                   double omega, hipStream_t st);
// One colour of the multicolour Gauss-Seidel: storage rows [row0, row0+count) of a
// colour-permuted SELL-64 matrix (row0 % 64 == 0), rowid = dof of each storage
// row (-1 pads); u[rowid] = (f - sum_{j != i} a_ij u_j) / a_ii in place.
hipError_t launch_sell_gs_color(int64_t n_storage, int max_width, const int64_t* soff,
                                const int32_t* scol, const double* sval, const int32_t* rowid,
                                int64_t row0, int64_t count, const double* f, double* u,
                                hipStream_t st);

// uH_zero (may be null): coarse solution vector zero-filled in the same pass
hipError_t launch_linear_restrict(int64_t n_h, int64_t n_H, const double* r, double* fH,
                                  double* uH_zero, hipStream_t st);
hipError_t launch_linear_prolong_add(int64_t n_h, int64_t n_H, const double* uH,
                                     double* uh, hipStream_t st);
// K-TensorRestrict / K-TensorProlong: the transfers of the full-coarsening hierarchies (host_setup.hpp:
// tensor_P) without a matrix.  dims = fine grid (x fastest; dim = 2: dims[2] == 1 is not coarsened);
// every coarsened axis must have at least 2 points and the fine level fewer than 2^31 - 2 rows, else
// hipErrorInvalidValue.  Bit-identical to the CSR SpMV with R / P (same terms, same order).
// mask: the coarsened axes (bit 0 = x, 1 = y, 2 = z; host_setup.hpp: tensor_P with a mask) -- 3 / 7
// for full coarsening; an axis outside the mask keeps its length (identity) and may have 1 point.
// sides: the natural boundary sides (bit 2a = low side of axis a, 2a + 1 = high side; host_setup.hpp:
// tensor_P with sides), 0 = every side Dirichlet; bits at or above 2 dim: hipErrorInvalidValue.
// periodic: the periodic axes (bit a = axis a; host_setup.hpp: tensor_P with periodic), 0 = none.  A
// periodic axis has no side bits and, where the mask coarsens it, an even length of at least 4; bits
// at or above dim: hipErrorInvalidValue.  With no coarsened periodic axis the launch is the one of
// periodic = 0, the same kernel and the same bits.
// f_H = R r, uH_zero (may be null) zero-filled in the same pass
hipError_t launch_tensor_restrict(int dim, const int64_t dims[3], uint32_t mask, uint32_t sides, uint32_t periodic,
                                  const double* r, double* fH, double* uH_zero, hipStream_t st);
// u_h = u_h + P u_H
hipError_t launch_tensor_prolong_add(int dim, const int64_t dims[3], uint32_t mask, uint32_t sides, uint32_t periodic,
                                     const double* uH, double* uh, hipStream_t st);
// K-AxisRestrict / K-AxisProlong: the transfers of a level that coarsens ONE axis with weights taken
// from its matrix (host_setup.hpp: axis_opdep_P), matrix-free.  dims = fine grid as above; axis: 0 = x,
// 1 = y, 2 = z (< dim, dims[axis] >= 2, else hipErrorInvalidValue).  W: the compact weights, 16-byte
// aligned -- the fine points with an even axis coordinate 2 q form a grid like dims with the axis
// shortened to m - floor(m / 2); point e of it (x fastest) has W[2 e] = w_lo (coarse q - 1) and
// W[2 e + 1] = w_hi (coarse q), 0.0 where the neighbour does not exist.  The weights are no powers
// of two: every product is rounded, then added in the order of the CSR SpMV with R / P (from +0.0,
// ascending column), so the bits are those of launch_csr(CSR_SPMV / CSR_SPMV_ADD) on R / P.
// periodic: the axis wraps (host_setup.hpp: axis_opdep_P with periodic; its length even and at least
// 4, else hipErrorInvalidValue): every even point has both weights, w_lo of fine 0 belongs to the
// last coarse point, and the ascending order changes at the seam alone -- the last coarse point adds
// fine 0 first, fine 0 adds its high neighbour first.  false: the open kernels, the same code as before.
// f_H = R r, uH_zero (may be null) zero-filled in the same pass
hipError_t launch_axis_restrict(int dim, const int64_t dims[3], int axis, bool periodic, const double* W,
                                const double* r, double* fH, double* uH_zero, hipStream_t st);
// u_h = u_h + P u_H
hipError_t launch_axis_prolong_add(int dim, const int64_t dims[3], int axis, bool periodic, const double* W,
                                   const double* uH, double* uh, hipStream_t st);
// x[j * stride] = +0.0 for j < count (count <= 64, else hipErrorInvalidValue)
hipError_t launch_zero_strided(double* x, int64_t stride, int count, hipStream_t st);
hipError_t launch_add_inplace(int64_t n, const double* x, double* y, hipStream_t st);
// *out = sum x_i (square=0) or sum x_i^2 (square=1); scratch: 1024 doubles
hipError_t launch_sum(int64_t n, const double* x, double* out, double* scratch, int square,
                      hipStream_t st);

// K-PCG: *out = sum x_i y_i (deterministic two-stage tree; scratch: 1024 doubles), and the
// two vector updates with alpha = *num / *den resp. beta = *num / *den formed on the device
hipError_t launch_dot(int64_t n, const double* x, const double* y, double* out, double* scratch,
                      hipStream_t st);
hipError_t launch_pcg_update_xr(int64_t n, const double* num, const double* den, double* x, double* r,
                                const double* p, const double* q, hipStream_t st);
hipError_t launch_pcg_update_p(int64_t n, const double* num, const double* den, double* p,
                               const double* z, hipStream_t st);
// K-Center: centre(v)_i = v_i - *sum / (double)n, *sum the device scalar of launch_sum(v, square = 0).
// launch_center: dst = centre(src) (dst may be src).  launch_center_dot: z = centre(z) and
// *out = sum r_i z_i of the centred z in one pass, the bits of launch_dot(r, centre(z)); scratch: 1024 doubles
hipError_t launch_center(int64_t n, const double* sum, const double* src, double* dst, hipStream_t st);
hipError_t launch_center_dot(int64_t n, const double* sum, double* z, const double* r, double* out,
                             double* scratch, hipStream_t st);

// In-graph neighbour exchange (K-Halo).  All pointers are device pointers; *_at_*
// and dst_* point into a neighbour's hipIpc-mapped arena.
struct HaloArgs {
  double* dst_prev; const double* src_prev; int64_t cnt_prev;
  double* dst_next; const double* src_next; int64_t cnt_next;
  uint32_t* my_free_from_prev; uint32_t* my_free_from_next;
  uint32_t* data_at_prev; uint32_t* data_at_next;
  uint32_t* my_data_from_prev; uint32_t* my_data_from_next;
  int32_t recv_prev, recv_next;
  uint32_t* timeout;
};
hipError_t launch_halo_exchange(const HaloArgs& a, hipStream_t st);
hipError_t launch_halo_ack(uint32_t* free_at_prev, uint32_t* free_at_next, hipStream_t st);
constexpr int GATHER_MAX_RANKS = 16;
struct GatherArgs {
  int32_t rank, world;
  const double* src; int64_t cnt, off;
  double* dst[GATHER_MAX_RANKS];          // every rank's full vector (own included)
  uint32_t* data_at[GATHER_MAX_RANKS];    // word [me] in rank g's DATA block
  uint32_t* free_at[GATHER_MAX_RANKS];    // word [me] in rank g's FREE block
  uint32_t* my_data_from;                 // my DATA block, one word per source rank
  uint32_t* my_free_from;                 // my FREE block, one word per destination rank
  uint32_t* timeout;
};
hipError_t launch_gather(const GatherArgs& a, hipStream_t st);
hipError_t launch_gather_ack(const GatherArgs& a, hipStream_t st);

struct LexDev {  // device copy of a LexSchedule
  int32_t block = 0, width = 0;
  int64_t n_slots = 0;
  const int32_t* row = nullptr;
  const int16_t* depth = nullptr;
  const int32_t* win_depth = nullptr;
  const int32_t* col = nullptr;
  const double* val = nullptr;
  const int16_t* src = nullptr;
};
// mode 0 SpGS, 1 reference "Jacobi" (forward GS), 2 SOR
hipError_t launch_gs_lex(const LexDev& S, const double* b, double* u, int mode, double omega,
                         hipStream_t st);

// Line-scan form of the lexicographic sweeps on a dictionary-coded matrix (K-GS-scan):
// chunks of C rows, the in-chunk chain u_k = c_k + q_k u_{k-1} solved by an affine scan.
// mode 0 SpGS update, 1 reference "Jacobi" (forward GS), 2 SOR.  ring: power of two.
void set_scan_typed(int on);  // K-GS-scan: per-type fast path on row-typed matrices (default on)
// s_old: scratch of n doubles (the sums over rows the sweep has not reached, formed by a
// parallel pre-pass).
// chunks of up to gs_scan_max_chunk() rows (else 1024): row-typed matrices whose rows have at most 4
// new-side entries besides the chain
bool gs_scan_long_chunks_ok(const DictRef& D);
int gs_scan_max_chunk();
hipError_t launch_gs_scan(int64_t n, const DictRef& D, const double* b, double* u, double* s_old,
                          bool backward, int mode, double omega, int C, int ring, hipStream_t st);

// m: lanes taking part (power of two > half-bandwidth, 4..64); sched_f/sched_b:
// per-(step, lane) L operands (host_setup: band_schedule); y: scratch, n doubles
hipError_t launch_band_solve(int64_t n, int m, const double* sched_f, const double* sched_b,
                             const double* dg, const double* f, double* y, double* x,
                             hipStream_t st, int cols = 1, int64_t cstride = 0);
// cols > 1 (the block cycle): one workgroup per right-hand side in the same launch, column c's
// f / y / x at c * cstride; cols = 1 is the single-vector launch (the same for K-BandChain and
// K-BandWide below)

// K-BandChain: narrow band (w <= 3), small n (<= 2048), everything in LDS; same bits as K-Band.
// cf / cb: n x w operands per step (host_setup.hpp: band_chain_schedule)
bool band_chain_ok(int64_t n, int64_t w);
hipError_t launch_band_chain(int64_t n, int w, const double* cf, const double* cb, const double* dg,
                             const double* f, double* x, hipStream_t st, int64_t n_h = 0,
                             const double* uh_in = nullptr, double* uh_out = nullptr, int cols = 1,
                             int64_t cstride = 0);
// Any half-bandwidth (K-BandWide): rows in blocks of 64; sched_f/sched_b hold per block a
// [w][64] panel of the operands that reach into earlier blocks followed by the block's own
// [64][64] triangle (host_setup: band_wide_schedule).  w + 64 <= 8192 (LDS ring).
hipError_t launch_band_wide(int64_t n, int64_t w, const double* sched_f, const double* sched_b,
                            const double* dg, const double* f, double* y, double* x,
                            hipStream_t st, int cols = 1, int64_t cstride = 0);

// Partitioned coarse solve (K-Spike); arrays as in host_setup.hpp: SpikeFactor.
struct SpikeArgs {
  int64_t n;
  int32_t w, c, P, m;
  int64_t sched_stride;
  const double *sched_f, *sched_b, *d, *V, *W, *Vt, *Wh;
  const double* f;
  double* x;
  double *G, *Z;   // scratch, n doubles each
  double *T, *H;   // scratch, P * max(w,1)
};
hipError_t launch_spike_solve(const SpikeArgs& a, hipStream_t st);

// K-Galerkin (setup): A_H = R (A P) for the linear interpolation pair, on CSR arrays that
// live on the device; count pass (fill = false: cnt[row]) / fill pass (orp = scanned
// counts) around launch_exclusive_scan.  Same entry order and bits as spgemm_csr.
hipError_t launch_exclusive_scan(int64_t n, const int32_t* counts, int32_t* offsets, int64_t* bsum,
                                 int64_t* total, hipStream_t st);
// general CSR x CSR product, Eigen's conservative order (count pass: cnt; fill pass: orp); rows
// of A with more than 32 entries set *overflow
hipError_t launch_spgemm(bool fill, int64_t n_rows, const int32_t* arp, const int32_t* acol,
                         const double* aval, const int32_t* brp, const int32_t* bcol, const double* bval,
                         int32_t* cnt, const int32_t* orp, int32_t* ocol, double* oval,
                         int32_t* overflow, hipStream_t st);
hipError_t launch_galerkin_ap(bool fill, int64_t n_h, int64_t n_H, const int32_t* arp,
                              const int32_t* acol, const double* aval, int32_t* cnt,
                              const int32_t* orp, int32_t* ocol, double* oval, hipStream_t st);
hipError_t launch_galerkin_rap(bool fill, int64_t n_h, int64_t n_H, const int32_t* prp,
                               const int32_t* pcol, const double* pval, int32_t* cnt,
                               const int32_t* orp, int32_t* ocol, double* oval, hipStream_t st);
// K-TensorGalerkin (setup): A_H = R (A P) for the full-coarsening pair of the fine grid `dims`
// (host_setup.hpp: tensor_P, R = P^T) from a general CSR(A) on that grid, without P, R or A P in
// memory; count pass (cnt[coarse row]) / fill pass (orp = scanned counts).  Same entry order and
// bits as galerkin_csr on the Kronecker operators, structural zeros included.  *overflow (zeroed
// by the caller) is set when a coarse row reaches more coarse columns than a lane group holds
// (16 in 2-D, 32 in 3-D): the result is then unusable and the caller takes the host product.
// mask, sides: the coarsened axes and the natural sides, as for launch_tensor_restrict.
// periodic: the periodic axes (tensor_P with periodic), every one of them whether this level
// coarsens it or not -- the wrap entries of A count on both; 0 launches the kernel without the seam.
hipError_t launch_tensor_galerkin(bool fill, int dim, const int64_t dims[3], uint32_t mask, uint32_t sides, uint32_t periodic,
                                  const int32_t* arp,
                                  const int32_t* acol, const double* aval, int32_t* cnt,
                                  const int32_t* orp, int32_t* ocol, double* oval, int32_t* overflow,
                                  hipStream_t st);
// K-AxisWeights (setup): the compact weights W of launch_axis_restrict from CSR(A_l) on the grid
// `dims`, for the level that coarsens `axis` (host_setup.hpp: axis_opdep_P's weight pass, same bits,
// -0.0 included).  W: 2 (n_l - n_{l+1}) doubles, 16-byte aligned, every one of them written.
// *first_bad (INT32_MAX before the launch) = the smallest row axis_opdep_row refuses.  n_l < 2^28.
// periodic: the solver's periodic axes.  When `axis` is one of them (its length even and >= 4) the
// collapse takes the distance mod m and every even point has both weights (axis_opdep_row with
// periodic, same bits); otherwise the kernel without the seam runs.
hipError_t launch_axis_weights(int dim, const int64_t dims[3], int axis, uint32_t periodic, const int32_t* arp,
                               const int32_t* acol, const double* aval, double* W, int32_t* first_bad, hipStream_t st);
// K-AxisGalerkin (setup): A_H = R (A P) for the one-axis pair with the weights W, count pass / fill
// pass and *overflow as for launch_tensor_galerkin.  Same entry order and bits as galerkin_csr on
// axis_P_from_weights(W) and its transpose; the structure is geometric (an entry for every
// neighbour that exists, zero weights included).  The count pass reads neither aval nor W.
// periodic: the solver's periodic axes, every one of them whether this level coarsens it or not (as
// for launch_tensor_galerkin); W and P are then axis_opdep_P's with periodic on a coarsened axis that
// wraps.  0 launches the kernel without the seam.
hipError_t launch_axis_galerkin(bool fill, int dim, const int64_t dims[3], int axis, uint32_t periodic,
                                const int32_t* arp, const int32_t* acol, const double* aval, const double* W,
                                int32_t* cnt, const int32_t* orp, int32_t* ocol, double* oval, int32_t* overflow,
                                hipStream_t st);
// K-AxisStrength (setup): out[a] = bits of max |a_ij| over the entries of CSR(A) on the grid `dims`
// whose column is the row's neighbour along axis a alone (host_setup.hpp: tensor_axis_strength,
// same bits); 0.0 when there is none.  out: 3 words, initialised by the launch.
hipError_t launch_axis_strength(int64_t n, int dim, const int64_t dims[3], const int32_t* rowptr, const int32_t* col,
                                const double* val, uint64_t* out, hipStream_t st);

// K-Setup: Grid generators and the dictionary encoder on the device (kernels.hip)
hipError_t launch_laplacian_count(int dim, int64_t n, int64_t n_last, int64_t N, int32_t* cnt, hipStream_t st);
hipError_t launch_laplacian_fill(int dim, int64_t n, int64_t n_last, int64_t N, const int32_t* rowptr, int32_t* col,
                                 double* val, double off, double diag, hipStream_t st);
// stats[0] = longest row (exact zeros skipped when prune), stats[1] = 1 when not bitwise
// symmetric (both zero-initialised by the caller); diag (optional) = a_ii
hipError_t launch_csr_inspect(int64_t n, const int32_t* rowptr, const int32_t* col, const double* val,
                              bool prune, int32_t* stats, double* diag, hipStream_t st);
// fail: 64 int32, zero-initialised: [0] = rows that did not encode, [1..62] = their indices
hipError_t launch_dict_encode(int64_t n, const int32_t* rowptr, const int32_t* col, const double* val,
                              bool prune, const int32_t* doff, const double* dval, int ntab, int words,
                              uint64_t* codes, int32_t* fail, hipStream_t st);
hipError_t launch_dict_types(int64_t n, const uint64_t* codes, int words, const uint64_t* rwords,
                             int ntypes, uint8_t* rtype, int32_t* fail, hipStream_t st);
// K-CsrCheck: rowptr[0] == 0, rowptr non-decreasing and within [0, nnz], columns in [0, n) and
// strictly ascending inside a row.  *first_bad (INT32_MAX before the launch) = first offending row.
hipError_t launch_csr_check(int64_t n, int64_t nnz, const int32_t* rowptr, const int32_t* col, int32_t* first_bad,
                            hipStream_t st);
// K-SellPack: upload_mat's panel layouts from a device CSR.  Count pass: kept[n] (row lengths after
// pruning), pslots[ceil(n / 64)] (64 * panel width), stats[3] zeroed by the caller = {longest kept
// row, 1 when 16-bit relative indices do not fit, most kept entries of a 256-row block}.  Fill pass:
// off32 = exclusive scan of pslots (widened into soff), scol int16 relative or int32 absolute.
hipError_t launch_sell_count(int64_t n, const int32_t* rowptr, const int32_t* col, const double* val, bool prune,
                             int32_t* kept, int32_t* pslots, int32_t* stats, hipStream_t st);
hipError_t launch_sell_fill(int64_t n, const int32_t* rowptr, const int32_t* col, const double* val, bool prune,
                            const int32_t* off32, int64_t* soff, bool idx16, void* scol, double* sval,
                            hipStream_t st);
// the CSR outcome: kept entries only, optr = exclusive scan of kept
hipError_t launch_csr_compact(int64_t n, const int32_t* rowptr, const int32_t* col, const double* val, bool prune,
                              const int32_t* optr, int32_t* ocol, double* oval, hipStream_t st);
// K-Transpose: CSR -> CSC of a square matrix.  cnt[n] zeroed by the caller, then scanned into cptr;
// cursor[n] zeroed; *overflow (zeroed) is set when a column has more than TRANSPOSE_MAX_COL entries
// (the result is then unusable).  The result equals the host transpose, structural zeros included.
constexpr int TRANSPOSE_MAX_COL = 32;
hipError_t launch_transpose_count(int64_t nnz, const int32_t* col, int32_t* cnt, hipStream_t st);
hipError_t launch_transpose_fill(int64_t n, const int32_t* rowptr, const int32_t* col, const double* val,
                                 const int32_t* cptr, int32_t* cursor, int32_t* orow, double* oval, int32_t* overflow,
                                 hipStream_t st);

// K-Block (kernels.hip): multi-right-hand-side forms for the block cycle.  Vectors are row-major
// panels of n x kp doubles (entry (i, j) at i * kp + j), kp in {1, 2, 4, 8, 16}; per column the
// operations of the single-vector kernels in the same order (same bits).  Plain CSR, lane = (row,
// column); modes CSR_RESID, CSR_JACOBI, CSR_SPMV, CSR_SPMV_ADD (f may be out), CSR_RSSQ.
hipError_t launch_block_csr(int mode, int kp, int64_t n, const int32_t* rowptr, const int32_t* col,
                            const double* val, const double* x, const double* f, double* out, double omega,
                            hipStream_t st);
hipError_t launch_block_csr_cheb(int kp, int64_t n, const int32_t* rowptr, const int32_t* col, const double* val,
                                 const double* x, const double* f, double* out, const ChebStep& c, hipStream_t st);
// linear_restrict / linear_prolong_add per column (uH_zero optional: zero-filled in the same pass)
hipError_t launch_block_restrict(int kp, int64_t n_h, int64_t n_H, const double* r, double* fH, double* uH_zero,
                                 hipStream_t st);
hipError_t launch_block_prolong_add(int kp, int64_t n_h, int64_t n_H, const double* uH, double* uh,
                                    hipStream_t st);
// to_panel: dst (n x kp) = src (n x k), columns k .. kp-1 zero; else dst (n x k) = the first k columns
hipError_t launch_block_pitch(int64_t n, int k, int kp, const double* src, double* dst, bool to_panel,
                              hipStream_t st);
// to_columns: dst[j * n + i] = src[i * kp + j]; else the inverse
hipError_t launch_block_columns(int kp, int64_t n, const double* src, double* dst, bool to_columns,
                                hipStream_t st);
// out[j] = sum_i x[i, j] (y null) or sum_i x[i, j] y[i, j], K-SumSq's tree per column; scratch: 1024 kp
hipError_t launch_block_sum(int kp, int64_t n, const double* x, const double* y, double* out, double* scratch,
                            hipStream_t st);
// K-PCG updates per column j with act[j] != 0: alpha = num[j] / den[j], x += alpha p, r -= alpha q;
// beta = num[j] / den[j], p = z + beta p
hipError_t launch_block_pcg_update_xr(int kp, int64_t n, const double* num, const double* den, const int32_t* act,
                                      double* x, double* r, const double* p, const double* q, hipStream_t st);
hipError_t launch_block_pcg_update_p(int kp, int64_t n, const double* num, const double* den, const int32_t* act,
                                     double* p, const double* z, hipStream_t st);
// K-Center per column j of a panel, m_j = sums[j] / (double)n (sums: launch_block_sum(v, null)):
// v = centre(v); z = centre(z) with out[j] = sum_i r[i, j] z[i, j] of the centred z (scratch: 1024 kp)
hipError_t launch_block_center(int kp, int64_t n, const double* sums, double* v, hipStream_t st);
hipError_t launch_block_center_dot(int kp, int64_t n, const double* sums, double* z, const double* r, double* out,
                                   double* scratch, hipStream_t st);

// K-LineBlock (kernels.hip): K-Line, K-LineX and K-LineSeam on the panels of K-Block.  The factors are
// the single-vector arrays (one entry per row, read once for the kp columns); r, y, u are n x kp
// panels and every panel index is 64-bit (n < 2^31, n kp may pass it).  Per (row, column) the
// expressions and their order are the single-vector kernels', so column j has their bits on column j.
// u += omega T^-1 r: launch_line_solve's kernels at pitch kp (lane = (segment, chain, column); (chain,
// column) or a workgroup per chain with kp walking lanes where line_few_chains(s); (row, column))
hipError_t launch_block_line_solve(int kp, const LineRef& L, const double* r, double* y, double* u, double omega,
                                   hipStream_t st);
int block_line_few_chunk(int kp);  // separators per LDS chunk of the few-chains walk at pitch kp
// x lines (stride kp in the panel): forward in place in r, then backward and update; lane = (run,
// column) walks linex_run(nx) rows straight from memory, 64 / kp runs to a wave, no LDS
hipError_t launch_block_linex_solve(int kp, const LineXRef& L, double* r, double* u, double omega, hipStream_t st);
// launch_line_seam per column: lane = (line, column); the x lines' sum in the W partials and the tree
// of seamx_kernel for the width W that line_seam_t picks for m
hipError_t launch_block_line_seam(int kp, const SeamRef& S, double* r, hipStream_t st);

// K-F32 (kernels.hip): the row kernels and transfers of the single-precision preconditioner.  mode:
// CSR_RESID, CSR_JACOBI or cheb_kernel_mode(first, last) (omega = the step's beta, dvec = its d);
// launch_csr_f32 also takes CSR_SPMV and CSR_SPMV_ADD (f may be out).  soff / scol (idx16 bit 0:
// 16-bit relative indices) and rowptr / col are the double matrix's arrays; x != out.
hipError_t launch_sell_f32(int mode, int64_t n, int idx16, const int64_t* soff, const void* scol, const float* sval,
                           const float* x, const float* f, float* out, float omega, float* dvec, float alpha,
                           hipStream_t st);
hipError_t launch_csr_f32(int mode, int64_t n, const int32_t* rowptr, const int32_t* col, const float* val,
                          const float* x, const float* f, float* out, float omega, float* dvec, float alpha,
                          hipStream_t st);
// K-DictF32: the same modes on a dictionary-coded matrix.  D is the DOUBLE matrix's view (codes or row
// types + word table, column offsets; D.dval is not read), tabv its pair table's values as floats
// (D.ntab of them).  hipErrorInvalidValue: x == out, a Chebyshev mode without dvec, n >= 2^30 - 1024
// (the byte offsets of x are 32-bit), or x / f / out / dvec not aligned to 4 R bytes, the row types
// not to R bytes, the code words not to 16 (R = rows per lane, 4 or 2).
hipError_t launch_dict_f32(int mode, int64_t n, const DictRef& D, const float* tabv, const float* x, const float* f,
                           float* out, float omega, float* dvec, float alpha, hipStream_t st);
// dst[i] = (float)src[i] / (double)src[i], round to nearest
hipError_t launch_to_f32(int64_t n, const double* src, float* dst, hipStream_t st);
hipError_t launch_to_f64(int64_t n, const float* src, double* dst, hipStream_t st);
// x[i] = +0.0f as a kernel: the float cycle's captured graph holds no memset node (solver.cpp:
// enqueue_f32_vcycle)
hipError_t launch_zero_f32(int64_t n, float* x, hipStream_t st);
// float instantiations of launch_linear_restrict / _prolong_add and launch_tensor_restrict / _prolong_add
hipError_t launch_linear_restrict_f32(int64_t n_h, int64_t n_H, const float* r, float* fH, float* uH_zero,
                                      hipStream_t st);
hipError_t launch_linear_prolong_add_f32(int64_t n_h, int64_t n_H, const float* uH, float* uh, hipStream_t st);
hipError_t launch_tensor_restrict_f32(int dim, const int64_t dims[3], uint32_t mask, uint32_t sides, uint32_t periodic, const float* r, float* fH, float* uH_zero,
                                      hipStream_t st);
hipError_t launch_tensor_prolong_add_f32(int dim, const int64_t dims[3], uint32_t mask, uint32_t sides, uint32_t periodic, const float* uH, float* uh,
                                         hipStream_t st);

}  // namespace amg_hip
