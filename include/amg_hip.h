/* =============================================================================
 * amg_hip.h -- C ABI of the MI355X-native V-cycle (libamg_hip.so)
 *
 * Drop-in boundary for the V-cycle hot path of jfdev001/algebraic-multigrid.
 * The reference is header-only C++ (no FFI of its own); these entry points are
 * what a binding of its public interface binds.  Each one cites the reference
 * interface it replaces (paths relative to the reference repository).
 * include/amg/ *.hpp is the C++ drop-in layer (AMG::Multigrid<> etc.) written on
 * top of exactly these functions; INTEGRATION.md shows both.
 *
 * Conventions
 *  - plain pointers + sizes, no C++/torch types; all indices int32 (Eigen's
 *    default StorageIndex), all values fp64 (the only EleType the reference
 *    instantiates, test/testlib.cpp throughout).
 *  - sparse matrices are COMPRESSED COLUMN (Eigen::SparseMatrix<double> default):
 *    colptr[cols+1], rowind[nnz] ascending inside a column, val[nnz].
 *  - every function returns an amg_hip_status; amg_hip_last_error() gives the
 *    thread-local message of the last failure.  The C++ layer re-throws
 *    AMG_HIP_EINVAL as std::invalid_argument with the reference's message text
 *    (multigrid.hpp:165-178, smoother.hpp:286-293).
 *  - there is NO CPU fallback: without a usable HIP device every compute entry
 *    point fails with AMG_HIP_EHIP.
 *  - one handle = one host thread at a time (the reference is not thread-safe
 *    either); different handles are independent.
 * ===========================================================================*/
#ifndef AMG_HIP_H
#define AMG_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  AMG_HIP_OK = 0,
  AMG_HIP_EINVAL = 1,       /* bad argument (-> std::invalid_argument)        */
  AMG_HIP_EHIP = 2,         /* HIP runtime / device failure                    */
  AMG_HIP_ENOMEM = 3,       /* host or device allocation failed                */
  AMG_HIP_EUNSUPPORTED = 4, /* valid request this build cannot run on device   */
  AMG_HIP_ECOMM = 5         /* RCCL failure (amg_hip_comm_*, the sharded cycles) */
} amg_hip_status;

/* Smoother plug-ins (smoother.hpp).  0-2 are the reference's three classes;
 * 3-7 are build-side additions the reference does not contain.   */
typedef enum {
  AMG_HIP_SM_SPGS = 0,          /* AMG::SparseGaussSeidel smoother.hpp:86-216:
                                   n_iters x (forward + backward lexicographic
                                   sweep), column-as-row walk, exact order      */
  AMG_HIP_SM_REF_JACOBI = 1,    /* AMG::Jacobi smoother.hpp:223-264 (an in-place
                                   forward Gauss-Seidel, row addressed)         */
  AMG_HIP_SM_SOR = 2,           /* AMG::SuccessiveOverRelaxation :271-373       */
  AMG_HIP_SM_JACOBI = 3,        /* true two-buffer weighted Jacobi              */
  AMG_HIP_SM_MULTICOLOR_GS = 4, /* symmetric multicolour Gauss-Seidel           */
  AMG_HIP_SM_CHEBYSHEV = 5,     /* Chebyshev polynomial in D^-1 A of degree
                                   cheb_degree on [cheb_lower G, cheb_upper G],
                                   G = Gershgorin bound of D^-1 A per level (rows
                                   of A); smoother_iters applications per leg,
                                   each cheb_degree Jacobi-shaped passes        */
  AMG_HIP_SM_LINE_JACOBI = 6,   /* line relaxation, Jacobi between the lines: with T
                                   = the entries of A at column offsets 0, +s and -s
                                   (tridiagonal on each of the min(s, n) chains of
                                   rows c, c + s, c + 2s, ...), one sweep is
                                   u <- u + omega T^-1 (f - A u), the residual taken
                                   from the old u throughout; smoother_iters sweeps
                                   per leg.  The stride s of a level comes from its
                                   matrix alone: with w(d) the sum of |a_ij| over
                                   the entries at distance d = |j - i| >= 1, s is
                                   the LARGEST d with w(d) >= (1 - 1e-9) max w (s = 1
                                   without off-diagonal entries; see
                                   amg_hip_line_stride).  On the hierarchies made by
                                   halving the flat index it relaxes the lines of
                                   the direction that is not coarsened.  omega must
                                   lie in (0, 2); the default 1.0 is a poor choice
                                   here, 0.7 is recommended (INTEGRATION.md has the
                                   table).  Meant for diagonally dominant operators:
                                   T is eliminated without pivoting, and setup
                                   refuses with AMG_HIP_EINVAL (level and row in the
                                   message) a pivot that is zero or not finite.
                                   T is symmetric when A is, so the V-cycle stays a
                                   valid PCG preconditioner.  Window solvers and slab
                                   sharding refuse it (AMG_HIP_EUNSUPPORTED); the
                                   block entry points do too unless
                                   amg_hip_set_block_lines(1) is in force.       */
  AMG_HIP_SM_LINE_ALT = 7       /* alternating-direction line relaxation, only on
                                   solvers that know their level grids
                                   (amg_hip_create_tensor, _tensor_dev,
                                   _poisson_tensor; every other constructor refuses
                                   it with AMG_HIP_EINVAL).  The directions of a
                                   level with grid (nx, ny, nz), x fastest, are its
                                   axes of length >= 2 in the order x, y, z, with
                                   strides 1, nx, nx ny (amg_hip_line_directions).
                                   One sub-sweep in direction a is
                                   u <- u + omega T_a^-1 (f - A u), the residual
                                   taken from the current u, T_a = the diagonal of A
                                   plus its entries at column offsets +-stride_a that
                                   join two points of the same grid line of that
                                   axis (an entry at +-1 across a line end, or at
                                   +-nx across a plane end, stays in A only): every
                                   grid line is its own tridiagonal system.  One
                                   application runs the directions in ascending
                                   order on the way down and in descending order on
                                   the way up, smoother_iters applications per leg,
                                   so the post-smoother is the adjoint of the
                                   pre-smoother and the V-cycle of a symmetric A is
                                   a symmetric PCG preconditioner.  A level without
                                   such an axis does weighted Jacobi.  omega in
                                   (0, 2), 0.8 recommended; pivots as for
                                   AMG_HIP_SM_LINE_JACOBI (level, direction and row
                                   in the message).  Refused where that one is
                                   (AMG_HIP_EUNSUPPORTED), and accepted by the block
                                   entry points under the same switch.           */
} amg_hip_smoother;

/* Device layout of the level matrices (results are bit-identical in all).    */
typedef enum {
  AMG_HIP_LAYOUT_AUTO = 0, /* DICT when the matrix qualifies, else SELL-64 unless
                              its padding exceeds 25 %, else CSR                 */
  AMG_HIP_LAYOUT_CSR = 1,  /* plain CSR, LDS-staged kernel (K-CSR)               */
  AMG_HIP_LAYOUT_SELL = 2, /* CSR sliced in 64-row lane-interleaved panels       */
  AMG_HIP_LAYOUT_DICT = 3  /* dictionary-coded rows (K-Dict): one byte per entry
                              indexing a table of the matrix's distinct
                              (column offset, value) pairs; needs <= 255 pairs
                              and rows of <= 16 entries, else falls back to SELL.
                              With <= 255 distinct rows the whole row is one byte
                              (amg_hip_set_row_types)                             */
} amg_hip_layout;

/* Options of amg_hip_create.  Zero-initialise, then amg_hip_default_options. */
typedef struct {
  int32_t smoother;        /* amg_hip_smoother; default AMG_HIP_SM_SPGS         */
  int32_t smoother_iters;  /* SmootherBase::n_iters (smoother.hpp:37); default 1
                              (= SparseGaussSeidel(), smoother.hpp:183-187)     */
  double omega;            /* SOR / weighted-Jacobi relaxation; default 1.0     */
  int32_t device;          /* HIP device ordinal; -1 = current device           */
  int32_t use_graph;       /* 1: replay the V-cycle as one hipGraph (default)   */
  int32_t stencil_transfers; /* 1 (default): when P/R are the built-in
                              LinearInterpolator, use the matrix-free stride-2
                              kernels (bit-identical to the CSR path)           */
  int32_t layout;          /* amg_hip_layout of the level matrices on the device  */
  int32_t host_only;       /* 1: build the hierarchy on the host only (no device is
                              touched); getters work, compute entry points fail.
                              Used by the row-block multi-GPU driver, where every
                              rank slices its own rows out of the hierarchy.       */
  int32_t keep_structural_zeros; /* 0 (default): device copies of the level matrices
                              drop entries that are exactly 0.0 (Eigen's Galerkin
                              product keeps them, 22 % of level 1); results are
                              bit-identical, the getters still return them.       */
  int32_t no_fusion;       /* 0 (default): the true-Jacobi V-cycle takes the first
                              pre-smoothing sweep of a coarse level, whose input is the
                              zero vector, from f and the diagonal alone.  Same
                              operations on the same values: bit-identical.       */
  int32_t fuse_prolong;    /* 1: apply the prolongation inside the first post-smoothing
                              Jacobi sweep (bit-identical; measured slower, off)  */
  int32_t fast_coarse_solve; /* 1: solve the coarsest system with the partitioned
                              (parallel) form of the banded LDL^T whenever it applies
                              (half-bandwidth <= 63): depth ~2c+P steps instead of n.
                              Same direct solve, different rounding order: agrees with
                              the sequential substitution to ~1e-14 relative, not bit
                              for bit.  Default 0 = by size: partitioned from 4096
                              coarsest rows on (see exact_coarse_solve).             */
  int32_t host_galerkin;   /* 1: build the Galerkin products R (A P) on the host instead of
                              on the device (same entries, same bits; the device path
                              is taken for LinearInterpolator operators only)        */
  int32_t keep_residual;   /* 1: keep the level residuals r = f - A u readable through
                              amg_hip_get_vec(level, 2).  The reference holds them as
                              private workspace without a getter (multigrid.hpp:107), so
                              by default (0) the fused residual+restriction kernel does
                              not store r on the levels where it runs, and reading it
                              there returns AMG_HIP_EINVAL.                            */
  int32_t exact_coarse_solve; /* 1: always the sequential substitution (bit-exact against
                              the row-oriented LDL^T solve of the oracle), whatever the
                              size of the coarsest level.  Default 0.                   */
  int32_t exact_gs;        /* SparseGaussSeidel / AMG::Jacobi / SOR (lexicographic sweeps,
                              smoother.hpp:148-174).  1: always the dependency-scheduled
                              exact kernel (bit-exact, one latency-bound workgroup).
                              0 (default): levels of more than 65536 rows whose matrix
                              is dictionary-coded with one chained lower neighbour run
                              the line-scan form (the in-line recurrence u_k = c_k +
                              q_k u_{k-1} solved by a parallel affine scan: same sweep,
                              different rounding order, ~1e-13 relative); smaller
                              problems keep the exact kernel.                          */
  int32_t cyclic_lines;    /* amg_hip_create_tensor_periodic / _periodic_dev with AMG_HIP_SM_LINE_ALT
                              only ("cyclic lines" at that constructor).  1: every line direction
                              along a periodic axis that has 3 points or more on its level is
                              solved as a cyclic tridiagonal system, wrap entries included.
                              Default 0: open lines, the earlier releases bit for bit.  Every
                              other constructor and smoother refuses 1 (AMG_HIP_EINVAL).
                              The field takes the four bytes of alignment padding that earlier
                              releases had in front of `stream`: the size of the struct and the
                              offset of every other field are unchanged, and natural_sides,
                              singular stay its last two fields.                             */
  void* stream;            /* hipStream_t to run on; NULL (default) = the solver creates
                              and owns a non-blocking stream.  A caller that already
                              orders its device work on a stream (torch's current
                              stream in the multi-GPU driver) passes it here so that
                              no host synchronisation is needed between the two.   */
  int32_t window;          /* 1: the solver is one rank's WINDOW of a sharded hierarchy
                              ("window sharding" below): its coarsest level is the level
                              the ranks all-gather, so it is neither factored nor solved
                              here; amg_hip_vcycle / solve / apply / pcg are refused and
                              the cycle runs by parts (amg_hip_window_run).  Default 0. */
  int32_t cheb_degree;     /* AMG_HIP_SM_CHEBYSHEV: degree k >= 1 of the polynomial, i.e. matrix
                              passes per application (default 2)                       */
  double cheb_lower;       /* AMG_HIP_SM_CHEBYSHEV: the interval [lo, hi] = [cheb_lower G,
                              cheb_upper G], G = max_i (sum_j |a_ij|) / |a_ii| of each
                              level; 0 < cheb_lower < cheb_upper (defaults 0.3, 1.0).
                              Step 0: d = (t - x) / theta, step s >= 1: rho_s = 1 /
                              (2 sigma - rho_{s-1}), d = rho_s rho_{s-1} d + 2 rho_s / delta
                              (t - x); x += d, with t the Jacobi quotient (f_i - sum_{j!=i}
                              a_ij x_j) / a_ii, theta = (hi + lo) / 2, delta = (hi - lo) / 2,
                              sigma = theta / delta, rho_0 = 1 / sigma.  A zero diagonal is
                              refused at setup (AMG_HIP_EINVAL).                        */
  double cheb_upper;       /* AMG_HIP_SM_CHEBYSHEV: upper end factor (default 1.0)    */
  int32_t natural_sides;   /* tensor constructors only ("natural boundary sides" below): 6-bit
                              mask of the sides of the box on which the operator carries NO
                              Dirichlet condition (Neumann, Robin, symmetry plane, outflow).
                              Bit 2a = the low side of axis a (x = 0, y = 1, z = 2), bit 2a + 1
                              its high side.  Default 0 = every side Dirichlet: the hierarchy
                              of the earlier releases bit for bit.  Every other constructor
                              refuses a non-zero value (AMG_HIP_EINVAL).                     */
  int32_t singular;        /* 1: the caller states that A is singular with the constant vector as
                              its null space (pure Neumann); needs every side of natural_sides
                              set.  The coarsest solve then pins its last unknown to 0.  Not
                              verified -- the caller's statement, as symmetry is for
                              amg_hip_pcg.  Default 0.                                        */
} amg_hip_options;

typedef struct amg_hip_solver amg_hip_solver; /* opaque; owns device memory    */

const char* amg_hip_last_error(void);
void amg_hip_default_options(amg_hip_options* o);

/* Layout used by amg_hip_default_options and by the stand-alone host-array
 * operations below (process-wide; tests flip it to run both kernels).         */
void amg_hip_set_default_layout(int32_t layout);

/* SELL-64 column indices as 16-bit offsets from the row's diagonal column when
 * every entry of a matrix is within +-32767 of it (10 instead of 12 bytes per
 * entry; bit-identical results).  Process-wide, default on.                    */
void amg_hip_set_index16(int32_t on);
/* Stream matrices larger than ~192 MB with non-temporal loads (process-wide, default
 * on): the once-read matrix then does not evict the x lines the gathers re-use.  */
void amg_hip_set_nontemporal(int32_t on);
/* K-Dict: give every XCD one contiguous run of row tiles, so that the +-bandwidth
 * re-reads of x hit the L2 that fetched them; on wide bands (3-D levels) the same slab of lines of
 * every grid plane instead (default on = 1; 2 = contiguous runs everywhere, the round-2 order;
 * 0 = plain order).  Tuning switch.                                                */
void amg_hip_set_xcd_mapping(int32_t on);
/* K-Dict second level: when a dictionary-coded matrix has at most 255 distinct rows, store
 * one byte per row into a table of code words instead of the code words themselves
 * (process-wide, default on; bit-identical results).  Applies to matrices uploaded
 * after the call.                                                                */
void amg_hip_set_row_types(int32_t on);
/* K-Dict rows per lane: 2 (default; 16-byte lane accesses) or 1.  Process-wide;
 * bit-identical results, a tuning / test switch.                                */
void amg_hip_set_dict_rows(int32_t rows_per_lane);
/* K-Dict: waves whose 128 rows all share one 7-point ({-M,-m,-1,0,1,m,M}) or 15-point
 * ({-M,-m,0,m,M} x {-1,0,1}) row type -- the interior of a 3-D level -- fetch x as aligned pairs
 * (7 / 15 loads per lane instead of 16 / 32 gathers) with the values from a per-type scalar table.
 * Process-wide, default on (AMG_HIP_DICT_STENCIL=0 in the environment turns it off);
 * bit-identical results, a tuning / test switch.                                                */
void amg_hip_set_dict_stencil(int32_t on);
/* K-Patch (temporal blocking of the 2+2 true-Jacobi cycle: a level's down-leg and up-leg in
 * one launch each over 2-D patches of the level) is used on levels of at least this many rows
 * (default 10^6; negative = never).  Process-wide, read when a solver is created: existing
 * solvers keep theirs.  Bit-identical results; tests set 0.                              */
void amg_hip_set_patch_min_rows(int64_t rows);

/* K-Patch per-tile row-type flags (patches whose rows all share one type skip the row-type
 * loads and the bounds checks) on / off; process-wide, read at launch.  Same bits either way. */
void amg_hip_set_patch_tile_flags(int32_t on);
/* K-Patch hand-over between two consecutive K-Patch levels: on (default), the down-leg of the
 * coarser level forms its first from-zero Jacobi sweep from the right-hand side it holds anyway,
 * and the finer level's down-leg stores that right-hand side alone instead of the sweep as well
 * (one vector less written and read per level pair).  Process-wide, read when a solver is
 * created.  Same bits either way: an A/B switch for tests and measurements.              */
void amg_hip_set_patch_xf(int32_t on);
/* K-Patch tall legs: on (default), the Jacobi legs that run two dependent stencil stages on the data
 * they load -- every up-leg and the down-legs of the levels >= 1 -- use tiles of 44 lines with two
 * halo rings of lines instead of 42 with three; the level-0 down-leg (three stages) keeps 42.  Off:
 * 42 lines everywhere.  Process-wide, read when a solver is created.  Same bits either way: an
 * A/B switch for tests and measurements.                                                      */
void amg_hip_set_patch_tall(int32_t on);
/* K-Patch column-typed tiles: on (default), a tile whose held rows all lie inside the matrix and whose
 * every held column has one row type over all held lines -- the tiles at the two ends of the grid lines,
 * which never consist of one row type -- is recognised at set-up (tile flag 254) and evaluated with a
 * sliding 3 x 3 window and the weights of the lane's type, instead of the per-entry tables of the general
 * path.  Off: no such flag is built.  Process-wide, read when a solver is created.  Same bits either
 * way: an A/B switch for tests and measurements.                                                    */
void amg_hip_set_patch_coltype(int32_t on);
/* K-Patch seam: on (default), amg_hip_vcycles(s, n) with n >= 2 -- and amg_hip_solve between two
 * residual checks -- runs the level-0 up-leg of one cycle and the level-0 down-leg of the next as ONE
 * launch, so the level-0 vector between two cycles is neither stored nor loaded again (25 n_0 bytes
 * less per cycle).  Taken where levels 0 and 1 are K-Patch Jacobi levels with the hand-over between
 * them, level 0 is a 5-point level, the cycle is whole (no slab, no window) and keep_residual and
 * no_fusion are off (the level-0 residual vector then serves as the second buffer of the handed-over
 * vector); a single cycle, amg_hip_apply and PCG run as before.  Process-wide, read when a solver is
 * created.  Same bits either way: an A/B switch for tests and measurements.                        */
void amg_hip_set_patch_seam(int32_t on);
/* K-BandChain (coarsest solve kind 3) on / off; process-wide, read when a solver is created.
 * Same bits either way: an A/B switch for tests and tuning.                             */
void amg_hip_set_band_chain(int32_t on);

/* K-Tail (the deepest levels of the 2+2 true-Jacobi cycle -- at most 4095 rows each --, the
 * coarsest solve and the way back up in ONE launch of one workgroup) on / off; process-wide, read
 * when a cycle is enqueued (a captured graph keeps what it was captured with).  Same bits either
 * way.  OFF by default (AMG_HIP_TAIL_FUSION=1 in the environment turns it on): on MI355X the one
 * launch takes as long as the launches it replaces.                       */
void amg_hip_set_tail_fusion(int32_t on);

/* K-Duo: two consecutive pair levels (l, l+1) of the 2+2 true-Jacobi cycle run their down-legs as ONE
 * launch and their up-legs as one, instead of one pair launch per level and leg.  Pairing is greedy
 * from the finest pair level; a leftover level, a level of K-Tail's range and a pair of levels the
 * kernels are not built for keep the pair form.  The finer level of a duo rests in its second buffer
 * after the cycle; amg_hip_get_vec / amg_hip_set_vec follow that.  Process-wide, read when a solver
 * is created; ON by default (AMG_HIP_PAIR_DUO=0 in the environment turns it off).  Same bits either
 * way, and amg_hip_cycle_must_move reports what the pair launches would have moved.              */
void amg_hip_set_pair_duo(int32_t on);
/* the other level of `level`'s duo, or -1 */
int32_t amg_hip_pair_duo_partner(const amg_hip_solver* s, int32_t level);
/* The row windows of a K-Duo tile of `tile_rows` rows (even, at most 510) of a level with
 * half-bandwidth hb_l over a level with half-bandwidth hb_l1: 31 numbers, (rows before the base, rows)
 * of the twelve windows -- down-leg: residual, sweep and right-hand side of l+1, residual, sweep and
 * input of l; up-leg: second sweep, first sweep and input of l+1, second sweep, first sweep and
 * input of l -- then the capacities of the down-leg's right-hand side of l+1, sweep and input of l and
 * of the up-leg's first sweep and input of l+1 and of l.  With t0 the tile's first row, level-(l+1)
 * windows start at ((t0 / 2) & ~1) - before, level-l windows of the down-leg at 2 ((t0 / 2) & ~1) -
 * before, those of the up-leg at t0 - before.  Returns 0 when every window is within its capacity, 1
 * otherwise or on a bad argument.  Host only: needs no device.                                    */
int32_t amg_hip_duo_windows(int32_t hb_l, int32_t hb_l1, int32_t tile_rows, int32_t* out);
/* What tile number `tile` of a K-Duo launch owns (the kernels' own function): out[0 .. 1] = its rows of
 * level l, out[2 .. 3] = of level l+1, out[4 .. 5] = of level l+2, each a half-open range before
 * clipping to the level's size.  A launch runs ceil(n_l / tile_rows) tiles.  Returns 0, or 1 on a bad
 * argument.  Host only.                                                                          */
int32_t amg_hip_duo_owned(int32_t tile, int32_t tile_rows, int32_t* out);
/* rows of level l per tile that the K-Duo launchers use under half-bandwidth hb_l: 254 or 510 */
int32_t amg_hip_duo_tile_rows(int32_t hb_l);

/* Both periodic _dev constructors build their hierarchies on the device instead of downloading to
 * the host constructor: amg_hip_create_tensor_periodic_dev (K-TensorGalerkin with the seam) and
 * amg_hip_create_tensor_opdep_periodic_dev (K-AxisWeights and K-AxisGalerkin with the seam).
 * Process-wide, read when a solver is created; default 0 (AMG_HIP_PERIODIC_DEVICE_SETUP=1 in the
 * environment turns it on).  The same solver bit for bit either way; amg_hip_setup_on_device tells
 * the two apart.                                                                                   */
void amg_hip_set_periodic_device_setup(int32_t on);

/* The single-precision entry points (amg_hip_apply_f32, amg_hip_pcg_mixed, amg_hip_f32_*) accept
 * solvers smoothed with AMG_HIP_SM_LINE_JACOBI and AMG_HIP_SM_LINE_ALT (K-LineF32: the line solve
 * kernels instantiated on float, on float copies of the double factors).  Process-wide, read whenever a
 * float entry point runs its checks; default 0 (AMG_HIP_F32_LINES=1 in the environment turns it on).
 * Off: those solvers are refused as before (AMG_HIP_EUNSUPPORTED).  No double entry point is touched
 * either way.                                                                                     */
void amg_hip_set_f32_lines(int32_t on);

/* The single-precision entry points (amg_hip_apply_f32, amg_hip_pcg_mixed, amg_hip_f32_*) accept
 * solvers with levels stored in the dictionary layout (K-DictF32: the dictionary row kernel on float
 * vectors; code words, row types and column offsets are the double matrix's own arrays, the only float
 * copy is the pair table's values, at most 255 floats per matrix).  Process-wide, read whenever a float
 * entry point runs its checks on a solver that has no float copies yet; default 0 (AMG_HIP_F32_DICT=1 in
 * the environment turns it on).  Off: those solvers are refused as before (AMG_HIP_EUNSUPPORTED).  A
 * solver first used with the switch on keeps working after it is turned off (its copies are made
 * once); a solver refused with it off is accepted once it is on (a refusal leaves nothing behind).  No
 * double entry point and no float result on SELL / CSR levels is touched either way.  With
 * amg_hip_set_dict_rows(1) the float kernel runs its other rows-per-lane form (4 instead of 2): same
 * bits, a test switch.                                                                             */
void amg_hip_set_f32_dict(int32_t on);

/* The block entry points (amg_hip_block_vcycles, _rss, _pcg, _must_move) accept solvers smoothed with
 * AMG_HIP_SM_LINE_JACOBI and AMG_HIP_SM_LINE_ALT, cyclic_lines included (K-LineBlock: the line solve
 * kernels on row-major panels, reading the solver's own double factors once for all columns; column j
 * keeps the bits of the single-vector path).  Process-wide, read whenever a block entry point runs its
 * checks; default 0 (AMG_HIP_BLOCK_LINES=1 in the environment turns it on).  Off: those solvers are
 * refused as before (AMG_HIP_EUNSUPPORTED).  No single-vector and no float entry point is touched
 * either way.                                                                                      */
void amg_hip_set_block_lines(int32_t on);

/* Number of usable HIP devices (0 when none; never fails). */
int amg_hip_device_count(void);

/* ---- AMG::Multigrid<double> (multigrid.hpp:151-244, ctor = SETUP) ----------
 * A (n x n CSC) and b are copied (multigrid.hpp:193,201).  Level sizes follow
 * n_H = (n_h+1)/2 - 1 (multigrid.hpp:127-130); transfer operators are the
 * built-in LinearInterpolator (interpolator.hpp:106-141) unless custom P/R are
 * given; coarse operators are Galerkin R*(A*P) in Eigen's summation order with
 * structural zeros kept (multigrid.hpp:219-223); the coarsest level is factored
 * (banded LDL^T, replaces Eigen::SimplicialLDLT multigrid.hpp:240-243).
 * Everything is uploaded; u_0 = 0.                                            */
amg_hip_status amg_hip_create(int64_t n, const int32_t* colptr,
                              const int32_t* rowind, const double* val,
                              const double* b, int32_t n_levels,
                              const amg_hip_options* opts,
                              amg_hip_solver** out);

/* Same, for a user InterpolatorBase subclass (interpolator.hpp:43-44): the C++
 * layer runs make_operators(n_h, n_H, level) on the host for every level and
 * hands over P_l (n_l x n_{l+1}) and R_l (n_{l+1} x n_l), l = 0..n_levels-2,
 * as arrays of CSC triples.  n_{l+1} is the reference's (n_l + 1) / 2 - 1 unless R_l says
 * otherwise: when its largest row index + 1 differs, that is the coarse size (operators of
 * another coarsening, e.g. the Kronecker products of amg_hip_create_tensor built by hand).  */
amg_hip_status amg_hip_create_custom(int64_t n, const int32_t* colptr,
                                     const int32_t* rowind, const double* val,
                                     const double* b, int32_t n_levels,
                                     const int32_t* const* P_colptr,
                                     const int32_t* const* P_rowind,
                                     const double* const* P_val,
                                     const int32_t* const* R_colptr,
                                     const int32_t* const* R_rowind,
                                     const double* const* R_val,
                                     const amg_hip_options* opts,
                                     amg_hip_solver** out);

/* Strength-based C/F coarsening (/root/reference README.md:104-109 names
 * Ruge-Stueben as the alternative it did not build: NO reference counterpart, pinned to the
 * oracle twin only).  Classical first-pass C/F splitting on the strength graph
 * (threshold `theta`, typically 0.25) with direct interpolation, R = P^T, Galerkin R(AP) in
 * the same summation order as the reference's chain; the hierarchy ends at `max_levels` or
 * where a level has at most `min_coarse` rows or stops coarsening (amg_hip_n_levels tells).
 * The same V-cycle (multigrid.hpp:263-305) then runs on it: general CSR transfer kernels,
 * the smoother of `opts`, banded LDL^T of whatever width on the coarsest level.          */
amg_hip_status amg_hip_create_rs(int64_t n, const int32_t* colptr, const int32_t* rowind,
                                 const double* val, const double* b, int32_t max_levels,
                                 double theta, int64_t min_coarse, const amg_hip_options* opts,
                                 amg_hip_solver** out);

/* Full coarsening of a structured grid (NO reference counterpart: the reference halves the flat
 * index, which coarsens the x axis only; this is its LinearInterpolator, interpolator.hpp:106-141,
 * applied per axis).  The caller supplies A on the grid dims = (nx, ny, nz), x fastest: dof =
 * (k ny + j) nx + i, n = nx ny nz; dim = 2 needs nz = 1 and leaves it alone.  Per axis of length m
 * the coarse length is floor(m / 2) -- not the reference's (m + 1) / 2 - 1, which for even m leaves
 * the last grid line without a coarse point -- and P1(m) is the m x floor(m / 2) matrix whose
 * column j holds 0.5, 1.0, 0.5 on rows 2j, 2j+1, 2j+2 (those < m).  P_l = P1(nz) (x) P1(ny) (x)
 * P1(nx) (Kronecker products; every entry a product of powers of two, hence exact), R_l = P_l^T,
 * A_{l+1} = R_l (A_l P_l) by the host Galerkin product in the summation order of
 * amg_hip_create_custom on the same P / R (bit-identical level matrices).  A level is possible
 * while every coarsened axis has at least 2 points; asking for more returns AMG_HIP_EINVAL with the
 * level in the message, as do n != nx ny nz and dim outside {2, 3}.  opts as for
 * amg_hip_create_custom (every smoother, host_only, the layouts), except opts->window = 1:
 * AMG_HIP_EUNSUPPORTED.  With opts->stencil_transfers (the default) the transfers run as the
 * matrix-free kernels K-TensorRestrict / K-TensorProlong (amg_hip_level_transfer_kind = 2), with
 * stencil_transfers = 0 as CSR SpMV with the uploaded P / R: the same bits either way.  The
 * patch / marching / pair / tail fusions of the flat hierarchy do not fire on these levels, and
 * amg_hip_slab_setup refuses (there are no K-Patch levels).                                   */
amg_hip_status amg_hip_create_tensor(int64_t n, const int32_t* colptr, const int32_t* rowind,
                                     const double* val, const double* b, int32_t dim,
                                     const int64_t* dims /* 3 */, int32_t n_levels,
                                     const amg_hip_options* opts, amg_hip_solver** out);
/* Semi-coarsening of a structured grid (NO reference counterpart): amg_hip_create_tensor with a
 * per-level AXIS MASK, bit 0 = x, bit 1 = y, bit 2 = z.  A masked axis of length m goes to
 * floor(m / 2) with P1(m), an unmasked one keeps its length with the identity: P_l = P_z (x) P_y (x)
 * P_x, R_l = P_l^T, A_{l+1} = R_l (A_l P_l).  Every weight is still a product of powers of two, so
 * the bit-for-bit statements of amg_hip_create_tensor carry over (level matrices equal
 * amg_hip_create_custom on the same P / R; transfer kind 2 and kind 0 give the same bits).  For
 * operators that are anisotropic along a grid axis -- stretched grids, thin layers, a diffusivity
 * that differs by direction -- on which full coarsening with a point smoother stalls: only the
 * strongly coupled axes are coarsened and the point smoothers (true Jacobi, Chebyshev, with their
 * block and float forms) stay effective; the price is operator complexity.
 * axis_masks != NULL: n_levels - 1 explicit masks; `theta` and `min_coarse` are ignored and the
 * solver has exactly n_levels levels.  AMG_HIP_EINVAL, with the level in the message, for a zero
 * mask, bit 2 when dim = 2, bits above 7 and a masked axis of fewer than 2 points.
 * axis_masks == NULL: the automatic rule, n_levels being a maximum.  On a level's grid w_a =
 * max |a_ij| over the entries whose column's grid coordinates differ from the row's by +-1 in axis
 * a and by 0 in the others (0 without such an entry); an axis is eligible when it has at least 2
 * points; an eligible axis a is coarsened iff w_a >= theta * max over the eligible b of w_b.  The
 * hierarchy ends at n_levels, at a level of at most `min_coarse` rows, or when no axis is eligible
 * (amg_hip_n_levels tells).  The rule does not depend on any order of evaluation.  theta must lie
 * in (0, 1] (0.5 is a good choice) and min_coarse be at least 1, else AMG_HIP_EINVAL.
 * Everything else as amg_hip_create_tensor: every smoother, AMG_HIP_SM_LINE_ALT included (the level
 * grids are known), host_only, the layouts; opts->window = 1: AMG_HIP_EUNSUPPORTED.  All argument
 * checks come before the device is touched.  amg_hip_get_level_dims, amg_hip_level_transfer_kind,
 * amg_hip_get_transfer and amg_hip_line_directions work on these solvers.                       */
amg_hip_status amg_hip_create_tensor_semi(int64_t n, const int32_t* colptr, const int32_t* rowind,
                                          const double* val, const double* b, int32_t dim,
                                          const int64_t* dims /* 3 */, int32_t n_levels,
                                          const int32_t* axis_masks /* n_levels - 1, or NULL */,
                                          double theta, int64_t min_coarse,
                                          const amg_hip_options* opts, amg_hip_solver** out);
/* Operator-dependent interpolation for a structured grid (NO reference counterpart).  Every level
 * coarsens exactly ONE grid axis, and the 1-D interpolation weights along that axis come from the
 * level's own matrix, so that P follows coefficients that jump by orders of magnitude from cell to
 * cell (layered media, composites), where the fixed weights of the other tensor constructors leave
 * the smooth error to the Krylov method.  Arrays, grid, options and argument checks are those of
 * amg_hip_create_tensor_semi, all before the device is touched; opts->window = 1:
 * AMG_HIP_EUNSUPPORTED.  Periodic axes: amg_hip_create_tensor_opdep_periodic (on a matrix with wrap
 * entries this constructor skips them -- their axis distance is m - 1 -- and P 1 != 1 along the seam).
 * axis_masks != NULL: n_levels - 1 masks of exactly one bit each (1, 2, or 4 when dim = 3);
 * `min_coarse` is ignored and the solver has exactly n_levels levels.  AMG_HIP_EINVAL with the level
 * in the message for a mask of several bits, a zero mask and a masked axis of fewer than 2 points.
 * axis_masks == NULL: on each level w is amg_hip_tensor_axis_strength of the level's matrix and
 * grid; an axis a < dim is eligible when it has at least 2 points; the eligible axis with the
 * largest w_a is coarsened, the lowest axis on a tie.  The hierarchy ends at n_levels, at a level of
 * at most `min_coarse` rows (min_coarse >= 1, else AMG_HIP_EINVAL) or when no axis is eligible
 * (amg_hip_n_levels tells).  The rule does not depend on any order of evaluation.
 * Grid: a masked axis of length m goes to floor(m / 2), coarse point J at fine coordinate 2 J + 1:
 * the geometry and the sparsity pattern of amg_hip_create_tensor_semi's P for the same mask.
 * Weights of level l, axis a: row i of A_l (the ROW, also for a nonsymmetric A), c its axis-a
 * coordinate; its entries are added in ascending column order into s_m, s_0, s_p (from +0.0) by the
 * axis-a coordinate c - 1, c, c + 1 of their column, whatever the column's other coordinates;
 * entries at another axis-a distance are skipped, structural zeros are added.  Odd c: the point is
 * coarse point (c - 1) / 2, one entry 1.0.  Even c: w_lo = (-s_m) / s_0 from coarse c / 2 - 1 when
 * c >= 2, w_hi = (-s_p) / s_0 from coarse c / 2 when c + 1 < m, one negation and one division each;
 * an entry is kept for every neighbour that exists, even when it comes out 0.0.  An s_0 that is
 * zero or not finite, or a weight that is not finite: AMG_HIP_EINVAL with level and row in the
 * message.  These weights are P1 in the interior of the constant-coefficient Laplacian (on a grid
 * line next to a Dirichlet side of ANOTHER axis the collapsed s_0 keeps that side's term: 1/3
 * instead of 1/2 on the 5-point model problem), 1.0 at a side without a Dirichlet term, and the
 * flux-continuous k-/(k- + k+), k+/(k- + k+) across a jump; so
 * opts->natural_sides does not enter them (it is validated and reported as on _tensor_semi and only
 * serves opts->singular, which pins the coarsest solve as there; amg_hip_set_mean_projection works).
 * R = P^T, A_{l+1} = R (A P) by the host Galerkin product in the summation order of
 * amg_hip_create_custom: the level matrices are those of amg_hip_create_custom on the P / R of
 * amg_hip_get_transfer, bit for bit.  Every smoother of _tensor_semi (AMG_HIP_SM_LINE_ALT included),
 * host_only and every layout work; so do amg_hip_get_level_dims, _get_level_axes, _get_transfer and
 * _line_directions.  With opts->stencil_transfers (the default) the transfers run matrix-free as
 * K-AxisRestrict / K-AxisProlong on a compact per-point weight array (amg_hip_level_transfer_kind =
 * 3), else as CSR SpMV with the uploaded P / R (kind 0): the same bits either way.  The float and
 * block cycles take their CSR kernels on these levels.                                            */
amg_hip_status amg_hip_create_tensor_opdep(int64_t n, const int32_t* colptr, const int32_t* rowind,
                                           const double* val, const double* b, int32_t dim,
                                           const int64_t* dims /* 3 */, int32_t n_levels,
                                           const int32_t* axis_masks /* n_levels - 1 single-axis masks, or NULL */,
                                           int64_t min_coarse, const amg_hip_options* opts, amg_hip_solver** out);
/* amg_hip_create_tensor_opdep on a grid with periodic axes (bit a of `periodic_axes` = axis a, as for
 * amg_hip_create_tensor_periodic): unit cells of composites and layered media, where the coefficient
 * jumps AND every axis wraps.  A has the wrap entries between the coordinates 0 and m - 1 of a
 * periodic axis.  periodic_axes = 0 gives amg_hip_create_tensor_opdep's solver bit for bit.
 * Weights on a level that coarsens a PERIODIC axis a of length m (even and at least 4; coarse length
 * m / 2, coarse point J at fine coordinate 2 J + 1 as before): the entries of row i are added in
 * ascending column order from +0.0 into s_m, s_0, s_p by (c_col - c) mod m = m - 1, 0, 1; every other
 * distance is skipped, structural zeros are added.  EVERY even c = 2 q has both neighbours: w_lo =
 * (-s_m) / s_0 from coarse (q - 1) mod (m / 2) and w_hi = (-s_p) / s_0 from coarse q, one negation and
 * one division each, both kept even when they come out 0.0 or -0.0; no slot of
 * amg_hip_get_axis_weights stands for a missing neighbour on such a level.  The rows of a column of
 * P ascend: column m / 2 - 1 of the axis holds fine 0 (w_lo(0)), fine m - 2 (w_hi(m - 2)) and fine
 * m - 1 (1.0) in that order, and amg_hip_get_transfer returns them so.  The refusals (s_0 zero or not
 * finite, a weight not finite) are _tensor_opdep's.  A periodic axis that a level does not coarsen
 * needs nothing (its wrap entries have distance 0 on the coarsened axis and go into s_0); a coarsened
 * axis that is not periodic keeps _tensor_opdep's rule bit for bit.  R = P^T and the host Galerkin
 * product as there: the level matrices are amg_hip_create_custom's on the P / R of
 * amg_hip_get_transfer, bit for bit.
 * The sums of the transfers run from +0.0 in ascending column order, which changes at the seam alone:
 * restriction, last coarse point: f = ((+0.0 + w_lo(0) r(0)) + w_hi(m-2) r(m-2)) + 1.0 r(m-1);
 * prolongation, fine point 0: t = (+0.0 + w_hi(0) u_H(0)) + w_lo(0) u_H(m/2 - 1).  Kind 3 (the PER
 * forms of K-AxisRestrict / K-AxisProlong) and kind 0 give the same bits.
 * axis_masks == NULL: _tensor_opdep's rule; an axis a < dim is eligible when it is not periodic and
 * has at least 2 points, or is periodic with an even length of at least 4.  Explicit masks: a masked
 * periodic axis of odd length or below 4 is AMG_HIP_EINVAL with the level in the message.
 * Argument checks, all before the device is touched: _tensor_opdep's in its words under this name,
 * then amg_hip_create_tensor_periodic's: periodic_axes negative or with bits at or above dim; a
 * natural_sides bit on a periodic axis; singular = 1 unless both side bits of every non-periodic
 * axis are set (all axes periodic with natural_sides = 0 is the fully periodic singular case, where
 * b needs a zero mean and amg_hip_set_mean_projection helps).  opts->window = 1:
 * AMG_HIP_EUNSUPPORTED.  opts->cyclic_lines = 1 stays AMG_HIP_EINVAL as on every constructor but
 * _tensor_periodic: AMG_HIP_SM_LINE_ALT relaxes OPEN lines on these solvers.
 * Everything else works as on _tensor_opdep: every smoother, every layout, host_only,
 * stencil_transfers = 0, amg_hip_set_axis_stencil(0), amg_hip_get_axis_weights, _get_level_axes,
 * _get_level_dims, _get_transfer, _line_directions, amg_hip_set_mean_projection;
 * amg_hip_get_periodic_axes reports the mask.  The float and block cycles take their CSR kernels on
 * these levels.  The coarsest operator of a periodic box has a wide band (the note at
 * amg_hip_create_tensor_periodic): coarsen until the coarsest level is small.                      */
amg_hip_status amg_hip_create_tensor_opdep_periodic(int64_t n, const int32_t* colptr, const int32_t* rowind,
                                                    const double* val, const double* b, int32_t dim,
                                                    const int64_t* dims /* 3 */, int32_t periodic_axes,
                                                    int32_t n_levels,
                                                    const int32_t* axis_masks /* n_levels - 1 single-axis masks, or NULL */,
                                                    int64_t min_coarse, const amg_hip_options* opts,
                                                    amg_hip_solver** out);
/* 0: solvers made by amg_hip_create_tensor_opdep from now on take transfer kind 0 even with
 * opts->stencil_transfers.  Process-wide, default 1, read when a solver is created.  Same bits
 * either way: an A/B switch for tests and measurements.                                          */
void amg_hip_set_axis_stencil(int32_t on);
/* The compact weights of `level` of a solver made by amg_hip_create_tensor_opdep (or _opdep_dev,
 * which downloads them from the device at the first call), 2 (n_l - n_{l+1})
 * doubles; also on host_only solvers.  The fine points whose coordinate on the level's axis is even,
 * c = 2 q, form a grid like the level's with that axis shortened to m - floor(m / 2); the point with
 * flat index e on it (x fastest) has W[2 e] = w_lo (its coarse neighbour q - 1) and W[2 e + 1] =
 * w_hi (coarse q), 0.0 where the neighbour does not exist (on a level of
 * amg_hip_create_tensor_opdep_periodic that coarsens a periodic axis both always exist, and w_lo of
 * q = 0 belongs to coarse m / 2 - 1).  AMG_HIP_EINVAL on the coarsest level
 * and for every other solver.                                                                     */
amg_hip_status amg_hip_get_axis_weights(const amg_hip_solver* s, int32_t level, double* W);
/* Natural boundary sides (opts->natural_sides, opts->singular; honoured by amg_hip_create_tensor,
 * _tensor_semi, _tensor_dev and _tensor_semi_dev).  P1(m) interpolates fine point 0 -- and fine point
 * m - 1 of an odd m -- from its one coarse neighbour with weight 0.5: linear interpolation towards a
 * zero boundary value, which is wrong on a side without a Dirichlet condition (P 1 != 1 there, so
 * the coarse grids cannot correct smooth error next to that side and the iteration count grows with
 * the grid).  P1N(m; lo, hi) is P1(m) with entry (0, 0) = 1.0 when `lo` is set and, for odd m, entry
 * (m - 1, m / 2 - 1) = 1.0 when `hi` is set; for even m `hi` changes nothing, fine point m - 1 being
 * a coarse point.  The pattern does not change and every weight is still a product of powers of
 * two, so all bit-for-bit statements of the tensor family carry over.  A level uses P_l = P_z (x)
 * P_y (x) P_x with P1N on the coarsened axes (an axis outside the level's mask keeps the identity),
 * R_l = P_l^T, A_{l+1} = R_l (A_l P_l) in the same summation order; the same side mask holds on every
 * level.  The matrix-free transfers, K-TensorGalerkin, the CSR transfers of stencil_transfers = 0,
 * the float cycle and the block cycle all honour it.
 * Set a bit for every side on which the discrete operator has no Dirichlet term (its boundary rows
 * sum to zero there as the interior rows do); leave it clear on Dirichlet sides.
 * opts->singular = 1 (needs all 2 dim bits): the constants are then in the null space of every
 * Galerkin operator, and the coarsest solve -- every kind, also in the float and the block cycle --
 * PINS THE LAST UNKNOWN: with n the coarsest size, x[n-1] = +0.0 and x[0 : n-1] solves the leading
 * principal (n-1) x (n-1) block by the same banded LDL^T (SPD when A is semidefinite with the
 * constants as its only null vector; the coarse right-hand side is consistent up to rounding because
 * 1^T R r = 1^T r, so the dropped equation holds by itself).  The last entry of the coarsest
 * right-hand side is zeroed on the stream just ahead of the solve and reads 0 after a cycle;
 * amg_hip_get_level_matrix still returns the true (singular) coarsest operator.  No mean projection is
 * applied by default: a cycle, amg_hip_pcg and the other solvers return a solution up to an additive
 * constant, and the right-hand side has to be consistent (zero mean for a symmetric A).  The PCG
 * drivers project when amg_hip_set_mean_projection(s, 1) is in force; amg_hip_center_vec centres a
 * level vector for the plain cycles.
 * AMG_HIP_EINVAL before the device is touched, the field named in the message: natural_sides negative
 * or with bits at or above 2 dim; natural_sides != 0 on amg_hip_create, _custom, _rs, _poisson,
 * _poisson_window and _poisson_tensor (its model problem is Dirichlet); singular outside {0, 1};
 * singular = 1 unless all 2 dim bits of natural_sides are set; singular = 1 with fewer than 2 levels
 * (asked for, or where the automatic semi-coarsening rule stops at level 0): the coarsest right-hand
 * side would be the caller's own b.  K-Tail (amg_hip_set_tail_fusion, off by default) is not taken
 * on a singular solver; its cycles run the unfused launches.                                      */
/* Side mask of a solver (opts->natural_sides of a tensor constructor); 0 on every other solver.  Also
 * on host_only solvers.                                                                          */
amg_hip_status amg_hip_get_natural_sides(const amg_hip_solver* s, int32_t* mask);
/* Periodic axes.  `periodic_axes` is a bit mask, bit a = axis a (1 = x, 2 = y, 4 = z): the operator
 * couples the first and the last point of such an axis (channel flows, annuli, doubly and triply
 * periodic boxes); those wrap entries are ordinary entries of A.  On a coarsened periodic axis of
 * even length m >= 4 the 1-D factor is P1per(m), m x m/2 with 0.5, 1.0, 0.5 on rows 2j, 2j+1,
 * (2j+2) mod m of column j: P1(m) plus the one entry (0, m/2 - 1) = 0.5, so that fine point 0 is
 * interpolated between coarse points 0 and m/2 - 1 and every row sums to 1.  A level uses P_l = P_z
 * (x) P_y (x) P_x with P1per on the coarsened periodic axes, P1N with the axis' side bits on the
 * other coarsened axes and the identity outside the level's mask; R_l = P_l^T, A_{l+1} = R_l (A_l
 * P_l) by the same host product in the same summation order; the same mask holds on every level.
 * An axis that is periodic but not coarsened on a level needs nothing, the wrap being in A.  The
 * weights are still products of powers of two: level matrices equal amg_hip_create_custom on the
 * same P / R bit for bit, transfer kind 2 (K-TensorRestrict / K-TensorProlong with the seam) and
 * kind 0 give the same bits, and the float cycle and the block cycle honour the mask.  The rows of
 * a column of P ascend (amg_hip_get_transfer): in the last column of a periodic axis row 0 is first.
 * axis_masks == NULL: full coarsening with exactly n_levels levels; otherwise n_levels - 1 explicit
 * masks as for amg_hip_create_tensor_semi.  The automatic rule of that constructor is not offered.
 * Everything else as amg_hip_create_tensor / _tensor_semi with explicit masks: every smoother
 * (AMG_HIP_SM_LINE_ALT included), every layout, host_only, stencil_transfers 0 / 1, natural_sides
 * and singular from `opts`.  periodic_axes = 0 gives the solver of those constructors bit for bit.
 * The smoothers see the level matrices only.  By default the line smoothers treat a wrap entry as
 * a coupling off the line, like any entry outside the tridiagonal part, and a line along a periodic
 * axis is relaxed as an open line.
 * Cyclic lines (opts->cyclic_lines = 1, AMG_HIP_SM_LINE_ALT only): on every level, each direction
 * along a periodic axis of length m >= 3 solves the cyclic tridiagonal T_a = the open T_a plus the two
 * wrap entries alpha = A[i0, i1], beta = A[i1, i0] of every grid line (first row i0, last row i1; 0
 * when absent).  Entries that wrap to a different line (the diagonal neighbours across the seam of a
 * 9- / 27-point level) stay in A only; at m = 2 the wrap edge is the ordinary edge and nothing
 * changes.  The solve is Sherman-Morrison on the open kernels: with gamma = -A[i0, i0], T' = the open
 * T_a with the diagonal d(i0) - gamma and d(i1) - alpha beta / gamma, u = gamma e(i0) + beta e(i1),
 * v = e(i0) + (alpha / gamma) e(i1), T_a = T' + u v^T.  Set-up keeps p = T'^-T v (8 B per row) and
 * den = 1 + v . T'^-1 u, gamma, beta (24 B per line); a sub-sweep computes r = f - A u, K-LineSeam
 * subtracts fac gamma and fac beta from r(i0) and r(i1) with fac = (p . r) / den of the line, and the
 * open solve with the factors of T' follows: u += omega T_a^-1 r.  A symmetric A keeps T_a symmetric,
 * so the cycle stays a symmetric preconditioner.  Pick it when the coupling is strong ALONG a periodic
 * axis: the open line leaves the mode that is constant along the line and oscillates across it
 * undamped.  A zero or non-finite pivot of T' or T'^T, or such a den, is
 * AMG_HIP_EINVAL (level, direction and row in the message).  A cyclic T_a that is singular in exact
 * arithmetic (a line with zero row sums and no coupling off the line) is the caller's error and is
 * NOT reliably detected: rounding can leave a tiny non-zero den.  AMG_HIP_SM_LINE_JACOBI knows no
 * grid lines and keeps open chains.  With periodic_axes = 0 the option is accepted and changes no
 * bit.  AMG_HIP_EINVAL before the device is touched, `cyclic_lines` named: a value outside {0, 1};
 * 1 on any other constructor; 1 with any other smoother.
 * The coarsest operator of a periodic box has a band as wide as the wrap, so its factorisation runs
 * the any-bandwidth substitution: coarsen until the coarsest level is small (a few hundred rows).
 * AMG_HIP_EINVAL before the device is touched, the argument or field named in the message: what
 * amg_hip_create_tensor / _tensor_semi check, in their words; periodic_axes negative or with bits
 * at or above dim; a coarsened periodic axis whose length on that level is odd or below 4 (the
 * level in the message); a natural_sides bit on a periodic axis, which has no sides; singular = 1
 * unless both side bits of every axis that is NOT periodic are set -- all axes periodic with
 * natural_sides = 0 is the fully periodic singular case.  opts->window = 1: AMG_HIP_EUNSUPPORTED. */
amg_hip_status amg_hip_create_tensor_periodic(int64_t n, const int32_t* colptr, const int32_t* rowind,
                                              const double* val, const double* b, int32_t dim,
                                              const int64_t* dims /* 3 */, int32_t periodic_axes,
                                              int32_t n_levels,
                                              const int32_t* axis_masks /* n_levels - 1, or NULL = full coarsening */,
                                              const amg_hip_options* opts, amg_hip_solver** out);
/* Periodic mask of a solver made by amg_hip_create_tensor_periodic / _periodic_dev; 0 on every other
 * solver.  Also on host_only solvers.                                                            */
amg_hip_status amg_hip_get_periodic_axes(const amg_hip_solver* s, int32_t* mask);
/* Axis mask of the transfers between `level` and `level` + 1 of a solver made by one of the tensor
 * constructors (the full-coarsening ones report 3 in 2-D and 7 in 3-D); also on host_only solvers.
 * AMG_HIP_EINVAL on the coarsest level and for every other solver.                              */
amg_hip_status amg_hip_get_level_axes(const amg_hip_solver* s, int32_t level, int32_t* axis_mask);
/* The w of the automatic rule of amg_hip_create_tensor_semi for a matrix on the grid `dims`, on
 * host arrays (CSC or CSR: the maxima are the same); no device is needed.                       */
amg_hip_status amg_hip_tensor_axis_strength(int64_t n, const int32_t* colptr, const int32_t* rowind,
                                            const double* val, int32_t dim, const int64_t* dims /* 3 */,
                                            double* w /* 3 */);
/* Grid of `level` (3 entries, x fastest) of a solver made by amg_hip_create_tensor; also on
 * host_only solvers.  AMG_HIP_EINVAL for every other solver.                                    */
amg_hip_status amg_hip_get_level_dims(const amg_hip_solver* s, int32_t level, int64_t* dims /* 3 */);
/* How the transfers between `level` and `level` + 1 run in the V-cycle: 0 = CSR SpMV with the
 * uploaded P / R, 1 = the reference's flat stride-2 kernels (LinearInterpolator operators with
 * opts->stencil_transfers), 2 = the tensor-product kernels of amg_hip_create_tensor, 3 = the
 * single-axis kernels with per-point weights of amg_hip_create_tensor_opdep (K-AxisRestrict /
 * K-AxisProlong; 0 on such a level with stencil_transfers = 0, after amg_hip_set_axis_stencil(0),
 * or when the level has 2^31 - 4 rows or more).  Also on host_only solvers (what a device solver
 * with the same options would run).                                                             */
amg_hip_status amg_hip_level_transfer_kind(const amg_hip_solver* s, int32_t level, int32_t* kind);

/* The same constructor for the reference's own model problem, A = Grid::laplacian(n) and
 * b = Grid::rhs(n) (grid.hpp:88-98,108-140; dim = 3: the 7-point analogue), with the built-in
 * LinearInterpolator -- SETUP ON THE DEVICE END TO END: the
 * matrix generator, the Galerkin chain, the dictionary encoder, the diagonal and the symmetry
 * check are kernels; no host copy of any level matrix is made unless a getter asks for it
 * (the right-hand side is evaluated on the host threads: its values are libm's exp()).
 * Identical hierarchy, identical results (tests compare level matrices and V-cycles bitwise
 * with amg_hip_create on Grid-generated arrays).  Options that need host structures -- exact
 * lexicographic schedules (exact_gs or small problems), multicolouring, non-dictionary
 * layouts, host_only -- silently take the host path: generate, then amg_hip_create.       */
amg_hip_status amg_hip_create_poisson(int32_t dim, int64_t n, int32_t n_levels,
                                      const amg_hip_options* opts, amg_hip_solver** out);

/* amg_hip_create_tensor for A = Grid::laplacian(n), b = Grid::rhs(n) on the n^dim grid (dim = 2
 * or 3, every axis n -> floor(n / 2) per level) with the SETUP ON THE DEVICE: the generator, the
 * Galerkin chain (K-TensorGalerkin: A_H = R (A P) from CSR(A) with neither P, R nor A P in memory,
 * in the summation order of the host product), the dictionary encoder, the diagonal, the symmetry
 * check and the Chebyshev bounds are kernels.  The solver is indistinguishable from
 * amg_hip_create_tensor on the host-generated arrays with the same options: levels, dims, level
 * matrices bit for bit (structural zeros included), transfers (rebuilt when a getter asks),
 * transfer kind 2, bounds, right-hand side (evaluated on the host threads: libm's exp()), and
 * every cycle, apply, PCG and block call.  No host copy of a level matrix is made unless a getter,
 * the block cycle or a panel upload asks for one: levels that do not take the dictionary (the
 * 27-entry rows of the 3-D coarse levels, a level that is not bitwise symmetric) go to the host
 * once, and the coarsest operator is factored there.  Device path: true Jacobi and Chebyshev.
 * Everything else silently takes the host path (generate, then amg_hip_create_tensor): host_only,
 * host_galerkin, stencil_transfers = 0, fuse_prolong, a layout other than AUTO / DICT, multicolour
 * GS, the lexicographic smoothers, the line smoother, n^dim >= 2^28, a product beyond int32
 * indexing.  amg_hip_setup_on_device tells the two apart.
 * AMG_HIP_EINVAL: dim outside {2, 3}, n < 2, more levels than the rule allows (the level in the
 * message, worded as by amg_hip_create_tensor), bad Chebyshev options; AMG_HIP_EUNSUPPORTED:
 * opts->window = 1.  These checks come before the device is touched.                            */
amg_hip_status amg_hip_create_poisson_tensor(int32_t dim, int64_t n, int32_t n_levels,
                                             const amg_hip_options* opts, amg_hip_solver** out);
/* amg_hip_create_tensor for a caller's matrix that already sits in DEVICE memory, with the SETUP
 * ON THE DEVICE.  A is in CSR (the rows of A, columns strictly ascending inside a row) -- NOT the
 * CSC arrays of the host constructors -- and b_dev holds n doubles.  Both are copied; the caller's
 * arrays are only read, on the solver's stream, and the call returns after a synchronisation.
 * The hierarchy is that of amg_hip_create_tensor on the CSC arrays of the same A and b with the
 * same options: levels, dims, level matrices bit for bit (structural zeros included), layouts
 * (amg_hip_level_layout), transfer kind 2, Chebyshev bounds, line strides, and every cycle, apply,
 * PCG and block call.  The level loop is amg_hip_create_poisson_tensor's; on top of it, levels that
 * do not take the dictionary are packed into SELL-64 panels or pruned CSR on the device
 * (K-SellPack, upload_mat's rule for opts->layout) and levels that are not bitwise symmetric are
 * transposed there (K-Transpose), so that no level matrix crosses to the host during set-up but the
 * coarsest operator for its factorisation.  Two per-level detours to the host remain: a column of
 * more than 32 entries on a level that is not bitwise symmetric, and panels of 2^31 slots or more.
 * Device path: true Jacobi, Chebyshev and the line smoother with stencil_transfers, every layout,
 * n_levels >= 2 and n < 2^28.  Everything else silently downloads the arrays, transposes them on
 * the host and calls amg_hip_create_tensor: host_only, host_galerkin, stencil_transfers = 0,
 * fuse_prolong, multicolour GS, the lexicographic smoothers, one level, a coarse row beyond
 * K-TensorGalerkin's lane group, a product beyond int32 indexing.  amg_hip_setup_on_device tells
 * the two apart.
 * Before the device is touched -- AMG_HIP_EINVAL: null pointers, dim outside {2, 3}, n != nx ny nz,
 * dim == 2 with nz != 1, more levels than the rule allows (the level in the message), bad smoother,
 * Chebyshev, line or layout options; AMG_HIP_EUNSUPPORTED: opts->window = 1.  Then the arrays are
 * checked by one kernel (K-CsrCheck: rowptr[0] == 0, rowptr non-decreasing, columns in [0, n) and
 * strictly ascending inside a row); a failure is AMG_HIP_EINVAL with the first offending row in
 * the message, and nothing else runs on such a matrix.  rowptr_dev[n] states the length of
 * col_dev / val_dev: the check reads nothing beyond it.                                          */
amg_hip_status amg_hip_create_tensor_dev(int64_t n, const int32_t* rowptr_dev, const int32_t* col_dev,
                                         const double* val_dev, const double* b_dev, int32_t dim,
                                         const int64_t* dims /* 3, host */, int32_t n_levels,
                                         const amg_hip_options* opts, amg_hip_solver** out);
/* amg_hip_create_tensor_semi for a caller's matrix in DEVICE memory (CSR, as for
 * amg_hip_create_tensor_dev), on top of that constructor's level loop: the Galerkin products run
 * as K-TensorGalerkin with the level's mask, and the automatic rule takes its w from K-AxisStrength,
 * a maximum of non-negative doubles and therefore the host's bits -- masks, dims, level matrices
 * and every cycle equal amg_hip_create_tensor_semi on the CSC arrays of the same A.  Same device
 * path, same silent fallbacks to the host constructor and same argument checks as
 * amg_hip_create_tensor_dev, plus those of amg_hip_create_tensor_semi; amg_hip_setup_on_device
 * tells the two paths apart.                                                                     */
amg_hip_status amg_hip_create_tensor_semi_dev(int64_t n, const int32_t* rowptr_dev, const int32_t* col_dev,
                                              const double* val_dev, const double* b_dev, int32_t dim,
                                              const int64_t* dims /* 3, host */, int32_t n_levels,
                                              const int32_t* axis_masks /* n_levels - 1, host, or NULL */,
                                              double theta, int64_t min_coarse,
                                              const amg_hip_options* opts, amg_hip_solver** out);
/* amg_hip_create_tensor_opdep for a caller's matrix in DEVICE memory (CSR, as for
 * amg_hip_create_tensor_dev), on top of that constructor's level loop.  On every level that is not
 * the last, K-AxisWeights makes the compact weights of amg_hip_get_axis_weights from the rows of the
 * level's CSR arrays, straight into the array K-AxisRestrict / K-AxisProlong read (no upload), and
 * K-AxisGalerkin forms A_{l+1} = R (A P) from CSR(A_l) and those weights with neither P, R nor A P in
 * memory, in the summation order of the host product and with its structure (an entry for every
 * neighbour that exists, zero weights included).  The automatic rule takes its w from
 * K-AxisStrength.  Transfer kind 3 on every level.  The host copies of the weights and of P / R are
 * made when amg_hip_get_axis_weights, amg_hip_get_transfer, a float or a block cycle ask for them.
 * natural_sides and singular are honoured as on the host constructor (they do not enter the
 * weights); amg_hip_set_mean_projection works.  The solver equals amg_hip_create_tensor_opdep's on the
 * CSC arrays of the same A with the same options bit for bit: axes, dims, weights (-0.0 included),
 * level matrices, and every cycle, apply, PCG, mixed and block call.
 * Device path: true Jacobi, Chebyshev, the line smoothers, every layout, n_levels >= 2, n < 2^28.
 * Everything else silently downloads the arrays, transposes them on the host and calls
 * amg_hip_create_tensor_opdep: the fallbacks of amg_hip_create_tensor_dev (host_only, host_galerkin,
 * stencil_transfers = 0, fuse_prolong, multicolour GS, the lexicographic smoothers, one level),
 * amg_hip_set_axis_stencil(0) (kind 0 needs CSR P / R), a coarse row that reaches more coarse
 * columns than K-AxisGalerkin's lane group holds (16 in 2-D, 32 in 3-D: 9- / 27-point levels fit),
 * a product beyond int32 indexing.  amg_hip_setup_on_device tells the two paths apart.
 * The argument checks are amg_hip_create_tensor_opdep's in the same words under this entry point's
 * name, plus null arrays, all before the device is touched; then K-CsrCheck as for
 * amg_hip_create_tensor_dev.  A row whose s_0 is zero or not finite, or whose weight is not finite,
 * is AMG_HIP_EINVAL with the host constructor's text (level and the smallest such row).           */
amg_hip_status amg_hip_create_tensor_opdep_dev(int64_t n, const int32_t* rowptr_dev, const int32_t* col_dev,
                                               const double* val_dev, const double* b_dev, int32_t dim,
                                               const int64_t* dims /* 3, host */, int32_t n_levels,
                                               const int32_t* axis_masks /* n_levels - 1 single-axis masks, host, or NULL */,
                                               int64_t min_coarse, const amg_hip_options* opts, amg_hip_solver** out);
/* amg_hip_create_tensor_opdep_periodic for a caller's matrix in DEVICE memory (CSR, as for
 * amg_hip_create_tensor_opdep_dev).  The argument checks of the host constructor in the same words
 * under this name, plus null arrays, before the device is touched; then K-CsrCheck, first and
 * whatever the switch says.
 * With amg_hip_set_periodic_device_setup(1): amg_hip_create_tensor_opdep_dev's level loop on the
 * device with the periodic mask.  K-AxisWeights with the seam collapses the rows of a coarsened
 * periodic axis by the axis distance mod m (every even point has both weights, kept whatever their
 * value), straight into the array the periodic forms of K-AxisRestrict / K-AxisProlong read;
 * K-AxisGalerkin with the seam forms A_{l+1} with R's last row of the axis (fine points 0, m - 2,
 * m - 1) and the wrap entries of A on every periodic axis, coarsened on the level or not.  Transfer
 * kind 3 on every level; the automatic rule leaves out a periodic axis that is odd or shorter than 4,
 * as on the host; natural_sides, singular and amg_hip_set_mean_projection are honoured as on the
 * host; cyclic_lines = 1 stays refused.  Same smoothers, layouts and silent fallbacks to the host
 * constructor as amg_hip_create_tensor_opdep_dev; amg_hip_setup_on_device reports 1 unless it fell
 * back.  A refused row is AMG_HIP_EINVAL with the host constructor's text under this name.
 * periodic_axes = 0 then gives amg_hip_create_tensor_opdep_dev's solver, built on the device.
 * With the switch off (the default): the arrays are downloaded, transposed on the host and given to
 * amg_hip_create_tensor_opdep_periodic -- the silent host path, always -- and
 * amg_hip_setup_on_device reports 0.
 * Either way the solver equals the host constructor's bit for bit: axes, dims, weights (-0.0
 * included), P, R, level matrices, and every cycle, apply, PCG, mixed and block call.            */
amg_hip_status amg_hip_create_tensor_opdep_periodic_dev(int64_t n, const int32_t* rowptr_dev, const int32_t* col_dev,
                                                        const double* val_dev, const double* b_dev, int32_t dim,
                                                        const int64_t* dims /* 3, host */, int32_t periodic_axes,
                                                        int32_t n_levels,
                                                        const int32_t* axis_masks /* n_levels - 1 single-axis masks, host, or NULL */,
                                                        int64_t min_coarse, const amg_hip_options* opts,
                                                        amg_hip_solver** out);
/* amg_hip_create_tensor_periodic for a caller's matrix in DEVICE memory (CSR, as for
 * amg_hip_create_tensor_dev).  The arguments are checked as by the host constructor, the arrays by
 * K-CsrCheck, first and whatever the switch says.
 * With amg_hip_set_periodic_device_setup(1): amg_hip_create_tensor_dev's level loop on the device
 * with the periodic mask -- the Galerkin products run as K-TensorGalerkin's periodic form (the seam
 * of a coarsened axis and the wrap entries of A on every periodic axis), with explicit axis_masks as
 * for amg_hip_create_tensor_semi_dev; natural_sides and singular are honoured as on the host, the
 * coarsest operator is factored on the host.  Same smoothers, layouts and silent fallbacks to the
 * host constructor as amg_hip_create_tensor_dev (among them a coarse row beyond the kernel's lane
 * group); amg_hip_setup_on_device reports 1 unless it fell back.
 * With the switch off (the default): the arrays are downloaded, transposed on the host and given to
 * amg_hip_create_tensor_periodic -- the silent host path, always -- and amg_hip_setup_on_device
 * reports 0.
 * Either way the solver equals the host constructor's bit for bit.                               */
amg_hip_status amg_hip_create_tensor_periodic_dev(int64_t n, const int32_t* rowptr_dev, const int32_t* col_dev,
                                                  const double* val_dev, const double* b_dev, int32_t dim,
                                                  const int64_t* dims /* 3, host */, int32_t periodic_axes,
                                                  int32_t n_levels,
                                                  const int32_t* axis_masks /* n_levels - 1, host, or NULL */,
                                                  const amg_hip_options* opts, amg_hip_solver** out);
/* *on = 1: the hierarchy was built by a device-only path (amg_hip_create_poisson,
 * amg_hip_create_poisson_window, amg_hip_create_poisson_tensor, amg_hip_create_tensor_dev,
 * amg_hip_create_tensor_semi_dev, amg_hip_create_tensor_opdep_dev, and amg_hip_create_tensor_periodic_dev
 * and amg_hip_create_tensor_opdep_periodic_dev under amg_hip_set_periodic_device_setup(1), when they
 * did not fall back),
 * 0: by the host constructor -- every other entry point and the silent fallbacks.  Also on
 * host_only solvers (0).                                                                        */
amg_hip_status amg_hip_setup_on_device(const amg_hip_solver* s, int32_t* on);

void amg_hip_destroy(amg_hip_solver* s); /* ~Multigrid, multigrid.hpp:135 */

/* One V-cycle, multigrid.hpp:263-305 (including the smoothing + residual on
 * the coarsest level).  Asynchronous on the solver's stream.      */
amg_hip_status amg_hip_vcycle(amg_hip_solver* s);
/* n back-to-back V-cycles (what bench.py times); returns after enqueueing.   */
amg_hip_status amg_hip_vcycles(amg_hip_solver* s, int32_t n);
/* Block until the solver's stream is idle. */
amg_hip_status amg_hip_sync(amg_hip_solver* s);

/* ---- row-block ("slab") sharding of one V-cycle over several GPUs ---------
 * The reference is a serial program (multigrid.hpp:263-305 walks whole levels); this is the
 * build's multi-GPU form of that loop.  Every rank creates the SAME solver (whole hierarchy,
 * full-size vectors) and then runs the K-Patch levels 0..levels-1 only over its own block of
 * grid lines plus `halo_lines` lines either side, recomputed redundantly, so that the whole
 * cycle needs two exchanges, both done by the caller (RCCL / torch.distributed) on the
 * solver's stream:
 *   1. before part 1: lines [line_begin - halo_lines, line_begin) and [line_end, line_end +
 *      halo_lines) of u0 from the two neighbouring ranks (their owned lines, same offsets);
 *   2. between parts 1 and 2: all-gather of f_gather, rank g contributing the entries
 *      [g, g+1) * chunk_lines * gather_pitch (equal blocks; the allocation has room for
 *      world of them, entries past gather_rows are padding);
 * part 2 (levels >= `levels`, coarse solve included) runs replicated on every rank.  After
 * part 3 each rank holds its own lines of the level-0 solution; per-row arithmetic is the
 * single-GPU cycle's, so the assembled solution equals it bit for bit.
 * amg_hip_slab_plan is the pure host arithmetic (no device): per slab level l the lines
 * [down_lo[l], down_hi[l]) the down-leg runs over and [up_lo[l], up_hi[l]) for the up-leg. */
#define AMG_HIP_SLAB_MAX_LEVELS 8
typedef struct amg_hip_slab_info {
  int32_t levels;      /* slab levels (0 .. levels-1); level `levels` is the gathered one   */
  int32_t halo_lines;  /* lines of u0 each neighbour supplies before a cycle                */
  int64_t lines;       /* grid lines (the same on every slab level: x-only coarsening)      */
  int64_t chunk_lines; /* lines per rank = ceil(lines / world); the last rank may own fewer  */
  int64_t line_begin, line_end; /* this rank's lines                                        */
  int64_t pitch0;       /* entries per line on level 0                                      */
  int64_t gather_pitch; /* entries per line on level `levels`                               */
  int64_t gather_rows;  /* rows of level `levels`                                           */
  int64_t down_lo[AMG_HIP_SLAB_MAX_LEVELS], down_hi[AMG_HIP_SLAB_MAX_LEVELS];
  int64_t up_lo[AMG_HIP_SLAB_MAX_LEVELS], up_hi[AMG_HIP_SLAB_MAX_LEVELS];
  double* u0;           /* device: level-0 solution, room for world*chunk_lines*pitch0      */
  double* f_gather;     /* device: rhs of level `levels`, room for world*chunk_lines*gather_pitch */
} amg_hip_slab_info;
/* AMG_HIP_EUNSUPPORTED when a rank would own fewer lines than the halo depth. */
amg_hip_status amg_hip_slab_plan(int64_t lines, int32_t rank, int32_t world, int32_t levels,
                                 amg_hip_slab_info* out);
/* max_levels < 0: every K-Patch level.  AMG_HIP_EUNSUPPORTED when the solver has none, and for
 * the Chebyshev and line smoothers (not sharded).                                          */
amg_hip_status amg_hip_slab_setup(amg_hip_solver* s, int32_t rank, int32_t world,
                                  int32_t max_levels, amg_hip_slab_info* info);
/* part 1: down-legs of the slab levels; 2: the replicated rest of the cycle (from the gathered
 * rhs); 3: up-legs of the slab levels.  Asynchronous on the solver's stream (one hipGraph each). */
amg_hip_status amg_hip_slab_run(amg_hip_solver* s, int32_t part);

/* ---- window sharding: row blocks with sharded STORAGE and SETUP ------------
 * The reference's flat-index coarsening (multigrid.hpp:127-130, interpolator.hpp:116-129)
 * coarsens the fast axis only, so the grid lines (2-D) / x-y planes (3-D) -- "units" -- of every
 * level coincide and a block of whole units is a consistent cut of the whole hierarchy.  Rank g
 * creates an ORDINARY solver on the principal submatrix of its WINDOW of units [unit_begin,
 * unit_end) = its owned units plus `halo` units either side (A = the rows and columns of
 * Grid::laplacian(n) in the window, b = the window of Grid::rhs(n); grid.hpp:88-140): because
 * the window starts at an even flat index, coarse dof j of the window is coarse dof j + offset
 * of the whole problem, the window's LinearInterpolator is the window of the global one, and
 * every Galerkin row R (A P) (multigrid.hpp:219-223) whose fine rows lie two units inside the
 * window has the same entries, summed in the same order, as the global row -- bit-identical.
 * Nothing of the global problem is ever assembled on a rank above the gathered level.
 * One V-cycle (multigrid.hpp:263-305) on `k` distributed levels:
 *   1. halo: `halo` units of the level-0 solution from each neighbour (their owned units);
 *   2. amg_hip_window_run(s, 1): the down-legs of levels 0..k-1 over the window, whatever the
 *      smoother (each sweep / colour stage / residual / transfer makes one more unit at either
 *      end of the window stale; the halo depth is chosen so that the owned units of f_k and
 *      what the up-legs need of u_l stay valid: window_vcycle.py: WindowPlan);
 *   3. all-gather of the owned units of f_k; the levels >= k (their own solver, built from the
 *      all-gathered rows of A_k) run replicated, coarse solve included;
 *   4. the window of u_k goes back into level k of the window solver;
 *      amg_hip_window_run(s, 3): the up-legs of levels k-1..0.
 * Per-row arithmetic is the single-GPU kernels', so the owned units of the result equal the
 * single-GPU cycle bit for bit (tests/test_window_gloo.py, tests/test_gpu_window.py).
 * amg_hip_create_poisson_window: options as amg_hip_create_poisson; `n_levels` = k + 1 (level k
 * is only a container for f_k / u_k: opts->window is forced to 1).  AMG_HIP_EUNSUPPORTED for
 * the Chebyshev and line smoothers (not sharded).                                          */
amg_hip_status amg_hip_create_poisson_window(int32_t dim, int64_t n, int64_t unit_begin,
                                             int64_t unit_end, int32_t n_levels,
                                             const amg_hip_options* opts, amg_hip_solver** out);
/* Line ranges (window-local grid lines) for the K-Patch legs of the distributed levels, or
 * NULL arrays: every leg runs over the whole window.  k = amg_hip_n_levels(s) - 1.           */
amg_hip_status amg_hip_window_setup(amg_hip_solver* s, const int64_t* down_lo,
                                    const int64_t* down_hi, const int64_t* up_lo,
                                    const int64_t* up_hi);
/* part 1: down-legs (u_0 .. f_k), part 3: up-legs (u_k .. u_0); one hipGraph each.           */
amg_hip_status amg_hip_window_run(amg_hip_solver* s, int32_t part);
/* Device pointer of a level vector (which as in amg_hip_get_vec) for zero-copy exchanges. */
amg_hip_status amg_hip_vec_dev_ptr(amg_hip_solver* s, int32_t level, int32_t which, void** ptr,
                                   int64_t* n);

/* The stream the solver's work is enqueued on (its own, or opts->stream). */
amg_hip_status amg_hip_get_stream(amg_hip_solver* s, void** stream);

/* ---- communicator: RCCL from inside the library --------------------------------
 * The reference is a serial program; this is how a C / C++ caller of the drop-in runs the sharded
 * V-cycle (multigrid.hpp:263-305 over row blocks) without Python.  librccl.so is opened at run
 * time (dlopen; AMG_HIP_EUNSUPPORTED when there is none).  Rank 0 calls amg_hip_comm_unique_id
 * and hands the 128 bytes to every rank by whatever bootstrap the application has (MPI_Bcast,
 * torch.distributed, a file); every rank then calls amg_hip_comm_create (collective).  One process
 * per GPU.  The sharded cycles below are ONE call each: everything -- grouped ncclSend / ncclRecv
 * of the halo, the captured legs, one ncclAllGather, the replicated rest -- is enqueued on the
 * solver's stream, nothing synchronises with the host.                                        */
#define AMG_HIP_COMM_ID_BYTES 128
typedef struct amg_hip_comm amg_hip_comm;
amg_hip_status amg_hip_comm_unique_id(uint8_t id[AMG_HIP_COMM_ID_BYTES]);
amg_hip_status amg_hip_comm_create(const uint8_t id[AMG_HIP_COMM_ID_BYTES], int32_t rank, int32_t world,
                                   int32_t device, amg_hip_comm** out);
void amg_hip_comm_destroy(amg_hip_comm* c);
int32_t amg_hip_comm_rank(const amg_hip_comm* c);
int32_t amg_hip_comm_world(const amg_hip_comm* c);
/* grouped send / recv with rank-1 and rank+1 (counts in doubles; a null pointer or a zero count
 * skips that direction); `stream` = hipStream_t                                                */
amg_hip_status amg_hip_comm_neighbor_exchange(amg_hip_comm* c, const double* send_prev, int64_t n_send_prev,
                                              double* recv_prev, int64_t n_recv_prev,
                                              const double* send_next, int64_t n_send_next,
                                              double* recv_next, int64_t n_recv_next, void* stream);
/* out = [the `count` doubles of rank 0 | of rank 1 | ...]; in == out + rank * count is allowed */
amg_hip_status amg_hip_comm_all_gather(amg_hip_comm* c, const double* in, double* out, int64_t count,
                                       void* stream);
/* One slab-sharded V-cycle (the slab section above): `info` is what amg_hip_slab_setup returned
 * for (amg_hip_comm_rank, amg_hip_comm_world).  With a communicator of one rank this is
 * amg_hip_vcycle cut into its three graphs: same bits.                                       */
amg_hip_status amg_hip_slab_cycle(amg_hip_solver* s, amg_hip_comm* c, const amg_hip_slab_info* info);
/* One window-sharded V-cycle (the window section above): `w` the window solver, `t` the solver of
 * the replicated levels >= k (built from the gathered rows of A_k), both on ONE stream.  All
 * offsets / counts in doubles:
 *   level-0 solution of the window: owned rows [own0_off, own0_end); send_prev_cnt of its first
 *   rows go to rank-1, send_next_cnt of its last rows to rank+1; recv_prev_cnt rows arrive below
 *   own0_off, recv_next_cnt rows from own0_end on;
 *   level k: owned rows [own_k_off, own_k_off + own_k_cnt) of the window's f_k are this rank's
 *   block (block_k doubles per rank, padded) of the all-gather; the window's u_k is rows
 *   [uk_off, uk_off + n) of the tail's solution.                                            */
typedef struct amg_hip_window_plan {
  int64_t own0_off, own0_end;
  int64_t send_prev_cnt, recv_prev_cnt, send_next_cnt, recv_next_cnt;
  int64_t own_k_off, own_k_cnt, block_k, uk_off;
} amg_hip_window_plan;
amg_hip_status amg_hip_window_cycle(amg_hip_solver* w, amg_hip_solver* t, amg_hip_comm* c,
                                    const amg_hip_window_plan* p);

/* Multigrid::solve(), multigrid.hpp:311-337: while (iter < n_iters && error >
 * tol) { vcycle(); if (++iter % every == 0) error = rss }.  error starts at 100.
 * *converged = (error <= tol).  Prints nothing (the C++ layer prints the
 * reference's "AMG converged after N iterations." line).                      */
amg_hip_status amg_hip_solve(amg_hip_solver* s, double tol, int64_t every,
                             int64_t n_iters, int64_t* iters, double* last_rss,
                             int32_t* converged);

/* ---- the V-cycle as a preconditioner (README.md:127 of the reference, its ref [7]: "a
 * single V-cycle used for preconditioner to get M^-1 v") ------------
 * amg_hip_apply: z = M^-1 v, i.e. ONE vcycle() (multigrid.hpp:263-305) started from the
 * zero vector with v as the level-0 right-hand side.  v_dev / z_dev are DEVICE pointers
 * (n_dofs(0) doubles, may alias each other); enqueued on the solver's stream; the solver's
 * own right-hand side and solution are left as they were.                             */
amg_hip_status amg_hip_apply(amg_hip_solver* s, const double* v_dev, double* z_dev);
/* Preconditioned conjugate gradients for A_0 x = b with M^-1 = amg_hip_apply, entirely on the
 * device (SpMV, dot products, updates; alpha / beta never leave it).  Starts from the current
 * level-0 solution, replaces it with the result.  Stops when ||b - A x||_2 <= rtol ||b||_2
 * (checked every iteration) or after max_iters.  The smoother must make the cycle a
 * symmetric operator: SparseGaussSeidel (forward + backward), true Jacobi or multicolour GS
 * with equal pre / post sweeps all do.  A is the reference's negative definite Laplacian
 * (grid.hpp:88-98): CG runs on it unchanged (r.z and p.Ap are both negative).            */
amg_hip_status amg_hip_pcg(amg_hip_solver* s, double rtol, int64_t max_iters, int64_t* iters,
                           double* relres);
/* ---- mean projection for singular solvers (K-Center; DESIGN.md: "Mean projection") --------------
 * For a symmetric A with the constants as its null space 1^T (b - A x) = 1^T b for every x: with a
 * right-hand side that is consistent only up to its boundary data the residual cannot fall below
 * |1^T b| / sqrt(n), the drivers cannot stop and the iterate grows along the constants.  With the
 * switch on, amg_hip_pcg, amg_hip_pcg_mixed and amg_hip_block_pcg (per column) run on the complement
 * of the constants (PETSc's MatNullSpace remedy).  centre(v) = v - m, m = S / (double)n with S the
 * library's two-stage tree sum of v, one divide and one subtract per entry.  The iteration is
 * amg_hip_pcg's with:  b~ = centre(b) in a work vector, ||b~||_2 in the stopping rule and
 * r = b~ - A x0;  z = centre(M^-1 r) after every preconditioner call, in the pass that forms r . z
 * (r is not centred again);  x = centre(x) on every way out, the early ones included.  The caller's b
 * is the level-0 right-hand side again on return, bit for bit (amg_hip_block_pcg never writes B).
 * Nothing else changes: amg_hip_apply, amg_hip_apply_f32, the cycles, amg_hip_solve and amg_hip_rss
 * keep their bits, and with the switch off the drivers issue the launches they always did.
 * Per solver, default 0; only stores a flag, so it works on host_only solvers too.  AMG_HIP_EINVAL:
 * a null solver, `on` outside {0, 1}, on = 1 on a solver not created with opts->singular = 1
 * (`singular` in the message).  on = 0 is accepted on every solver.  Not for a nonsymmetric A, whose
 * left null vector is not the constants.                                                          */
amg_hip_status amg_hip_set_mean_projection(amg_hip_solver* s, int32_t on);
amg_hip_status amg_hip_get_mean_projection(const amg_hip_solver* s, int32_t* on);
/* v = centre(v) on a level vector (which: 0 = u, 1 = f), enqueued on the solver's stream, on any
 * device solver whatever the switch says: amg_hip_vcycles and amg_hip_solve do not project, a caller
 * who iterates with plain cycles centres f once with this.  AMG_HIP_EINVAL: level out of range,
 * `which` outside {0, 1}, a host_only solver.                                                     */
amg_hip_status amg_hip_center_vec(amg_hip_solver* s, int32_t level, int32_t which /* 0 = u, 1 = f */);

/* AMG::rss(A_0, u_0, b), common.hpp:17-27 (device tree reduction; agrees with
 * the sequential sum to ~1e-15 relative). */
amg_hip_status amg_hip_rss(amg_hip_solver* s, double* out);

/* ---- block (multi-right-hand-side) cycles on the solver's hierarchy ---------------------
 * F, U, B, X: DEVICE arrays of n_dofs(0) x k doubles, ROW-major (entry (i, j) at [i*k + j], i.e.
 * a contiguous torch tensor of shape (n_0, k)), 16-byte aligned, 1 <= k <= 16.  Work is enqueued
 * on the solver's stream.  Column j of every result has the bits of the single-vector entry point
 * on column j (vcycle() after set_vec(0, u / f, column j); rss(); pcg()).  The solver's own level
 * vectors are not touched.  Argument checks, in this order: null pointers, k outside 1..16,
 * n_cycles < 0, a misaligned pointer, bad rtol / max_iters -> AMG_HIP_EINVAL; a window solver or a
 * smoother other than AMG_HIP_SM_JACOBI / AMG_HIP_SM_CHEBYSHEV -> AMG_HIP_EUNSUPPORTED; then the
 * device (a host_only solver fails there).  With amg_hip_set_block_lines(1) the smoother check also
 * accepts AMG_HIP_SM_LINE_JACOBI and AMG_HIP_SM_LINE_ALT (cyclic_lines included); every other check
 * and its place in the order stay.  The first call builds plain CSR copies of the level
 * matrices that are not CSR already and n_l x kp panels per level (kp = k rounded up to a power
 * of two; the line smoothers take one more panel per level); with use_graph one captured graph per
 * kp.                                                                                          */
amg_hip_status amg_hip_block_vcycles(amg_hip_solver* s, int32_t k, const double* F, double* U,
                                     int32_t n_cycles);           /* U in/out: n_cycles V-cycles */
amg_hip_status amg_hip_block_rss(amg_hip_solver* s, int32_t k, const double* F, const double* U,
                                 double* out /* host, k */);      /* amg_hip_rss per column     */
/* k independent PCG recurrences (amg_hip_pcg's, step for step, from X) that share every SpMV and
 * every block V-cycle; a column that has stopped is frozen.  X receives the result; iters[j] and
 * relres[j] (host arrays of k, may be null) are amg_hip_pcg's per column.                     */
amg_hip_status amg_hip_block_pcg(amg_hip_solver* s, int32_t k, const double* B, double* X,
                                 double rtol, int64_t max_iters,
                                 int64_t* iters /* host, k */, double* relres /* host, k */);
/* Bytes one block cycle's launches have to move on k columns: every matrix once per launch (CSR:
 * 12 B per entry + 4 B per row), every vector 8 k bytes per row (padded columns not counted). */
amg_hip_status amg_hip_block_must_move(amg_hip_solver* s, int32_t k, double* bytes);

/* ---- single-precision preconditioner ("Single-precision preconditioner") -------------
 * The V-cycle of amg_hip_apply with every level vector, every level matrix value and every transfer
 * in float, as M^-1 of a PCG whose SpMV, dot products, updates and stopping rule stay in double.  CG
 * only needs a fixed, symmetric, reasonably accurate M^-1; the outer iteration keeps fp64 accuracy.
 * The path owns float copies of the matrix VALUES (SELL-64 panel offsets and 16- / 32-bit indices and
 * CSR row pointers / columns are shared with the double matrices) and float level vectors, made at
 * the first call and freed with the solver; the coarsest system is solved in double with the
 * existing factor.  The solver's own level vectors, right-hand side and solution are never touched,
 * and no existing entry point changes its results.  Not bitwise against the double cycle, but every
 * step is the float32 restatement of tests/f32_twin.py bit for bit: each row summed in ascending column
 * order from a fixed start with separate, correctly rounded multiplies, adds and divisions, the
 * transfers in the row order of the CSR R / P, the coarsest solve the double solve between two
 * roundings.  Deterministic, and use_graph = 0 / 1 give the same bits.
 * v is not scaled: entries of v below about 1e-30 in magnitude lose bits to float denormals, and
 * above 3e38 overflow.  Harmless for rtol >= 1e-12 on right-hand sides of ordinary magnitude.
 *
 * Checks, in this order, before the device is touched: AMG_HIP_EINVAL null pointers; AMG_HIP_EINVAL
 * bad rtol / max_iters (amg_hip_pcg_mixed); AMG_HIP_EUNSUPPORTED a window solver; AMG_HIP_EUNSUPPORTED
 * a smoother other than AMG_HIP_SM_JACOBI / AMG_HIP_SM_CHEBYSHEV; AMG_HIP_EUNSUPPORTED a one-level
 * solver.  Then a host_only solver fails (AMG_HIP_EINVAL), then AMG_HIP_EUNSUPPORTED for a level
 * stored in the dictionary layout (the level in the message),
 * unless amg_hip_set_f32_dict(1) is in force: create the solver with layout = AMG_HIP_LAYOUT_SELL, or
 * turn that switch on.
 *
 * With amg_hip_set_f32_lines(1) the smoother check also accepts AMG_HIP_SM_LINE_JACOBI and
 * AMG_HIP_SM_LINE_ALT (cyclic_lines included); every other check and its place in the order stay.
 * The line solves run in float on float copies of the double factors (made on the device at the
 * first float call with to_f32; there is no float elimination): half of the 72 B (2-D) or 120 B
 * (3-D) per row and level that the double factors of AMG_HIP_SM_LINE_ALT take, 24 B per row for
 * AMG_HIP_SM_LINE_JACOBI.  One application differs from amg_hip_apply's by 1e-7 to 4e-5 relative,
 * the strongly anisotropic operators at the upper end.
 *
 * amg_hip_apply_f32: z = M32^-1 v.  v_dev / z_dev: DEVICE pointers to n_dofs(0) doubles (may alias);
 * v is rounded to float, one float V-cycle from zero runs, the result is widened into z.  Enqueued on
 * the solver's stream.                                                                          */
amg_hip_status amg_hip_apply_f32(amg_hip_solver* s, const double* v_dev, double* z_dev);
/* amg_hip_pcg step for step (same arguments, same contract: starts from the level-0 solution,
 * leaves the result there, the right-hand side is b again) with amg_hip_apply_f32's cycle as M^-1. */
amg_hip_status amg_hip_pcg_mixed(amg_hip_solver* s, double rtol, int64_t max_iters, int64_t* iters,
                                 double* relres);
/* Bytes the launches of one amg_hip_apply_f32 have to move: per SELL entry 4 + w (w = 2 or 4 index
 * bytes) and 8 per panel, CSR 8 per entry + 4 per row pointer, every float vector pass 4 per row; the
 * coarsest solve and the conversions around it and around the cycle in their own widths.  A dictionary
 * level (amg_hip_set_f32_dict): n_rows + 256 * 8 * words + 8 * ntab with row types, 8 * words * n_rows +
 * 8 * ntab without (words = 1 or 2 code words per row, ntab = the distinct (column offset, value) pairs
 * of the matrix): amg_hip_level_layout's matrix_stream_bytes less 4 * ntab. */
amg_hip_status amg_hip_f32_must_move(amg_hip_solver* s, double* bytes);
/* TEST HOOKS on the float cycle, the float counterparts of amg_hip_get_vec / amg_hip_set_vec /
 * amg_hip_level_op: they let a test pin single steps of amg_hip_apply_f32 bit for bit and are not
 * meant for applications.  All three run amg_hip_apply_f32's checks in the order above (the first
 * of them, AMG_HIP_EINVAL, also for a level out of range, a bad `which`, an `op` the level does not
 * have), then make the float copies if this is the first float call.
 * amg_hip_f32_get_vec / amg_hip_f32_set_vec: n_dofs(level) floats to / from HOST memory; which: 0 = u,
 * 1 = f, 2 = r.  The coarsest level has u and f only (which = 2 there: AMG_HIP_EINVAL).  Both
 * synchronise the solver's stream.  After amg_hip_apply_f32 the vectors hold what the cycle left on
 * every level (level 0's f: v rounded to float, level 0's u: z before it is widened).
 * amg_hip_f32_level_op: one step of the float cycle on the float vectors -- the very launches
 * amg_hip_apply_f32 makes for it -- eagerly on the solver's stream; op as amg_hip_level_op's:
 *   0 smooth (smoother_iters sweeps, or applications of the Chebyshev polynomial)  level < L-1
 *   1 r_l = f_l - A_l u_l                                                          level < L-1
 *   2 u_{l+1} = 0 and f_{l+1} = R_l r_l                                            level < L-1
 *   3 u_l = u_l + P_l u_{l+1}                                                      level < L-1
 *   4 widen f_L, the solver's double coarse solve, round into u_L                  level = L-1 */
amg_hip_status amg_hip_f32_get_vec(amg_hip_solver* s, int32_t level, int32_t which, float* out_host);
amg_hip_status amg_hip_f32_set_vec(amg_hip_solver* s, int32_t level, int32_t which, const float* in_host);
amg_hip_status amg_hip_f32_level_op(amg_hip_solver* s, int32_t level, int32_t op);
/* TEST HOOKS on the float line smoothers (amg_hip_set_f32_lines).  Same checks as the three above
 * (AMG_HIP_EINVAL first: null pointers, a level out of range, d outside 0..2), then AMG_HIP_EINVAL for a
 * solver without a line smoother or a d the level does not have.  With a line smoother the coarsest
 * level (small, and the only one that can have a single row) keeps a float matrix, r and factors too,
 * so both hooks take every level, as amg_hip_level_op does (not a coarsest level stored in the
 * dictionary layout: AMG_HIP_EINVAL).
 * amg_hip_f32_line_subsweep: one sub-sweep on the float vectors of `level` with the launches the cycle
 * makes for it: r = f - A u (into the float r), K-LineSeam where direction d is cyclic, then
 * u += omega T_d^-1 r by K-LineX (which leaves its forward values in r) or K-Line.  d: the index among
 * the level's directions (axes of length >= 2 in the order x, y, z); AMG_HIP_SM_LINE_JACOBI and a
 * level without a direction: d = 0.  `reverse` names the leg (0 down, 1 up); a single sub-sweep is
 * the same on both.
 * amg_hip_f32_line_factors: the float K-LineX factors dl, ip, cp of `level` (n_dofs(level) floats each)
 * to HOST memory; AMG_HIP_EINVAL where the level has no x direction.                               */
amg_hip_status amg_hip_f32_line_subsweep(amg_hip_solver* s, int32_t level, int32_t d, int32_t reverse);
amg_hip_status amg_hip_f32_line_factors(amg_hip_solver* s, int32_t level, float* dl, float* ip, float* cp);

/* Getters, multigrid.hpp:339-354. */
int32_t amg_hip_n_levels(const amg_hip_solver* s);
int64_t amg_hip_get_n_dofs(const amg_hip_solver* s, int32_t level);
int64_t amg_hip_get_level_nnz(const amg_hip_solver* s, int32_t level);
/* get_coefficient_matrix(level): CSC copy out (arrays sized by the caller). */
amg_hip_status amg_hip_get_level_matrix(const amg_hip_solver* s, int32_t level,
                                        int32_t* colptr, int32_t* rowind,
                                        double* val);
/* which: 0 = P_level (n_l x n_{l+1}), 1 = R_level.  Returns nnz (<0: error). */
int64_t amg_hip_get_transfer_nnz(const amg_hip_solver* s, int32_t level, int32_t which);
amg_hip_status amg_hip_get_transfer(const amg_hip_solver* s, int32_t level,
                                    int32_t which, int32_t* colptr,
                                    int32_t* rowind, double* val);
/* which: 0 = get_soln, 1 = get_rhs, 2 = residual vector (multigrid.hpp:107).
 * Synchronises the stream, then copies n_dofs(level) doubles to/from host.    */
amg_hip_status amg_hip_get_vec(amg_hip_solver* s, int32_t level, int32_t which,
                               double* out);
amg_hip_status amg_hip_set_vec(amg_hip_solver* s, int32_t level, int32_t which,
                               const double* in);
/* Device-side copy between a level vector of the solver and caller-owned
 * DEVICE memory (n_dofs(level) doubles), enqueued on the solver's stream:
 * to_solver = 1 copies src -> solver vector, 0 copies solver vector -> dst.
 * which as in amg_hip_get_vec.  Lets a host that owns device buffers (the
 * multi-GPU driver's agglomerated coarse part) feed a right-hand side and take
 * the solution without a host round trip.                                      */
amg_hip_status amg_hip_copy_vec_dev(amg_hip_solver* s, int32_t level, int32_t which,
                                    void* dev_ptr, int32_t to_solver);
/* Zero-fill a level vector on the solver's stream. */
amg_hip_status amg_hip_zero_vec(amg_hip_solver* s, int32_t level, int32_t which);

/* Device layout the level's operator was uploaded in (amg_hip_layout, never AUTO)
 * and the bytes of its matrix stream (indices + values, or codes + table) that
 * one sweep reads -- what the format actually moves, next to the CSR-formula
 * figure of amg_hip_cycle_bytes.  host_only solvers: EINVAL.                    */
amg_hip_status amg_hip_level_layout(const amg_hip_solver* s, int32_t level, int32_t* layout,
                                    int64_t* matrix_stream_bytes);

/* Half-bandwidth of the factored coarsest operator. */
int64_t amg_hip_coarse_halfbw(const amg_hip_solver* s);
/* Which device form of the coarsest solve (multigrid.hpp:287-288) the solver uses:
 * 0 = one-wave sequential substitution (half-bandwidth <= 63, bit-exact),
 * 1 = partitioned / parallel (fast_coarse_solve or >= 4096 rows),
 * 2 = blocked sequential substitution for any half-bandwidth (bit-exact),
 * 3 = LDS-resident scalar recurrence for half-bandwidth <= 3 and <= 2048 rows (bit-exact;
 *     the coarsest level of a deep hierarchy).                                        */
int32_t amg_hip_coarse_solve_kind(const amg_hip_solver* s);
/* Multicolour smoother: colour of every dof of `level` (n_dofs int32) and the
 * colour count, so a CPU twin can replay the same colouring.                   */
amg_hip_status amg_hip_get_colors(const amg_hip_solver* s, int32_t level,
                                  int32_t* color, int32_t* n_colors);

/* Single steps of the V-cycle on one level, for a host that has to interleave its
 * own code with them: the C++ layer runs a USER-DEFINED SmootherBase subclass on
 * the host (vectors go device -> host -> smooth() -> device) and
 * everything else here.  op:
 *   0 smooth with the solver's built-in smoother           (multigrid.hpp:268,300)
 *   1 residual r_l = f_l - A_l u_l                          (:272-274)
 *   2 u_{l+1} = 0 and f_{l+1} = R_l r_l                     (:278-282)
 *   3 u_l = u_l + P_l u_{l+1}                               (:294-296)
 *   4 coarsest solve u_L = A_L^-1 f_L (level must be L-1)   (:287-288)        */
amg_hip_status amg_hip_level_op(amg_hip_solver* s, int32_t level, int32_t op);

/* AMG_HIP_SM_CHEBYSHEV: the interval [*lo, *hi] the smoother of `level` uses (cheb_lower and
 * cheb_upper times the level's Gershgorin bound of D^-1 A).  Also on host_only solvers (the
 * host setup computes the bounds without a device).  AMG_HIP_EINVAL for other smoothers.   */
amg_hip_status amg_hip_cheb_bounds(const amg_hip_solver* s, int32_t level, double* lo, double* hi);

/* AMG_HIP_SM_LINE_JACOBI: the stride s of `level` (the rule in the enum's comment).  Also on
 * host_only solvers, where the host computes it; the device rule gives the same integer.
 * AMG_HIP_EINVAL for other smoothers.                                                      */
amg_hip_status amg_hip_line_stride(const amg_hip_solver* s, int32_t level, int64_t* stride);

/* AMG_HIP_SM_LINE_ALT: the directions of `level`: *n_dir of them (0 .. 3) and their strides in
 * ascending order in strides[0 .. *n_dir) (the rest 0).  Also on host_only solvers.
 * AMG_HIP_EINVAL for other smoothers.                                                      */
amg_hip_status amg_hip_line_directions(const amg_hip_solver* s, int32_t level, int32_t* n_dir,
                                       int64_t strides[3]);

/* AMG_HIP_SM_LINE_ALT: the axes of `level` whose lines are solved cyclically (opts->cyclic_lines):
 * bit a = axis a, as in periodic_axes; 0 with cyclic_lines = 0, and for an axis with fewer than 3
 * points on the level.  Also on host_only solvers.  AMG_HIP_EINVAL for other smoothers.       */
amg_hip_status amg_hip_line_cyclic(const amg_hip_solver* s, int32_t level, int32_t* axis_mask);

/* Sum over levels of the algorithmic HBM bytes of one V-cycle (SURVEY 8(d)
 * formulae) and the per-sweep bytes of level 0; used by bench.py.  A cyclic sub-sweep
 * (opts->cyclic_lines) adds K-LineSeam's 16 B per row (p, r read) and 40 B per line (den, gamma,
 * beta read; two entries of r written).                                        */
amg_hip_status amg_hip_cycle_bytes(const amg_hip_solver* s, double* cycle_bytes,
                                   double* fine_sweep_bytes);

/* Bytes the launches of ONE V-cycle have to move: for every launch what that kernel reads and
 * writes once in the layout it really streams (dictionary: 1 B row type per row; K-Patch leg:
 * 25 n + 24 n_H down, 25 n + 8 n_H up; SELL / CSR: indices + values; vectors 8 B per entry),
 * summed while the cycle is enqueued.  part 0 = the whole cycle (bench.py divides it by the
 * measured time per cycle: the whole-cycle fraction of the HBM roof), 1 / 2 / 3 = the parts of
 * amg_hip_slab_run / amg_hip_window_run once they have run.  part 0 describes ONE STAND-ALONE cycle
 * whatever amg_hip_vcycles runs, so bench.py's whole_cycle fraction is quoted on the stand-alone
 * cycle's bytes; part 4 = one steady-state cycle of amg_hip_vcycles(s, n >= 2): with the K-Patch
 * seam (amg_hip_set_patch_seam) the seam launch (25 n_0 + 16 n_1) and levels 1 .. L-1, i.e. part 0
 * less 25 n_0; without it, part 0.                                                             */
amg_hip_status amg_hip_cycle_must_move(amg_hip_solver* s, int32_t part, double* bytes);

/* Measurement hook for bench.py: launches the level-0 smoother sweep kernel
 * (the dominant kernel of a V-cycle) n_launches times back to back on the
 * solver's own stream, each launch bracketed by a pair of HIP events on that
 * stream, and returns the average / minimum launch duration in milliseconds.
 * AMG_HIP_SM_JACOBI: one launch = one sweep over level 0 (K-Patch: the level's down-leg);
 * AMG_HIP_SM_CHEBYSHEV: one middle step of the polynomial over level 0 (u -> tmp, d read and
 * written), or step 0 when the degree has no middle step (1 or 2);
 * AMG_HIP_SM_LINE_JACOBI, AMG_HIP_SM_LINE_ALT: refused (AMG_HIP_EUNSUPPORTED; a sweep is several launches);
 * AMG_HIP_SM_MULTICOLOR_GS: the first launch of the symmetric pass (K-Patch form: two colour
 * stages over the level; K-Strip form: the level's whole down-leg, which like the K-Patch launch
 * also rewrites f and u of level 1; colour kernels: colour 0).  The level-0 solution is restored
 * afterwards.                                                                  */
amg_hip_status amg_hip_profile_fine_sweep(amg_hip_solver* s, int32_t n_launches,
                                          double* avg_ms, double* min_ms);
/* Lines of the tiles the V-cycle of this solver launches on `level` for its down-leg (leg 0) or
 * up-leg (leg 1): 42 or 44 on a K-Patch level, 0 where the level is no K-Patch level.  leg 2: of the
 * seam launch amg_hip_vcycles(s, n >= 2) runs on level 0 (38), 0 where this solver runs none.   */
int32_t amg_hip_patch_leg_lines(const amg_hip_solver* s, int32_t level, int32_t leg);
/* The launch form the cycle plan gives `level` on its down-leg and its up-leg (DESIGN.md section 4,
 * "The cycle plan"): of the cycle enqueued last, before the first one of the cycle that would run.  */
enum {
  AMG_HIP_LEG_NONE = 0,        /* no launch of its own (the coarsest level when r is not kept; host_only) */
  AMG_HIP_LEG_PLAIN = 1,       /* the smoother's own launches, then the transfers                      */
  AMG_HIP_LEG_PAIR = 2,        /* two sweeps of a small level in one launch                            */
  AMG_HIP_LEG_DUO_FINE = 3,    /* K-Duo: the finer level of a duo                                      */
  AMG_HIP_LEG_DUO_COARSE = 4,  /* K-Duo: the coarser level                                             */
  AMG_HIP_LEG_PATCH = 5,       /* K-Patch: the whole leg in one launch                                 */
  AMG_HIP_LEG_MC_PATCH = 6,    /* multicolour smoother: colour stages as patch launches                */
  AMG_HIP_LEG_MC_STRIP = 7,    /* multicolour smoother: K-Strip, the whole leg as one strip launch     */
  AMG_HIP_LEG_TAIL_HEAD = 8,   /* K-Tail: this level .. L-2, the solve and the way back in one launch  */
  AMG_HIP_LEG_IN_TAIL = 9      /* a level inside that launch                                           */
};
/* AMG_HIP_EINVAL for a level the solver does not have; a host_only solver reports none on both legs. */
amg_hip_status amg_hip_level_leg_form(const amg_hip_solver* s, int32_t level, int32_t* down, int32_t* up);
/* The K-Strip launches of `level`: rows per strip T, strips (workgroups) per launch, colour stages of
 * a leg, and the halo rows a strip loads on either side on the down-leg ((stages + 1) half-bandwidths:
 * the residual needs one more) and on the up-leg (stages half-bandwidths).  The LDS window of a launch
 * is T + 2 halo + 2 rows.  AMG_HIP_EINVAL where the plan runs `level` in another form.              */
amg_hip_status amg_hip_strip_geometry(const amg_hip_solver* s, int32_t level, int32_t* T, int32_t* tiles,
                                      int32_t* stages, int32_t* halo_down, int32_t* halo_up);
/* Tiles of `level` by class, for the launches with `rings` halo rings (2: tiles of 44 lines, 3: 42, 5: the
 * seam launch's, 38): out[0] = tiles of one row type, out[1] = column-typed tiles, out[2] = general
 * tiles.  AMG_HIP_EINVAL where the level is no K-Patch level or has no tiles of that geometry.        */
amg_hip_status amg_hip_patch_tile_classes(amg_hip_solver* s, int32_t level, int32_t rings, int64_t* out);
/* Name of the kernel amg_hip_profile_fine_sweep times (as rocprofv3 prints it, without the
 * namespace), the number of Jacobi sweeps over level 0 one launch of it performs, and the
 * bytes one launch has to move (what the kernel reads and writes once: SURVEY 8(d)'s CSR
 * formula for the CSR / SELL layouts; row types + f + x + out for the dictionary-coded one;
 * for the K-Patch down-leg additionally f_H, the first coarse sweep and the coarse diagonal).
 * On a K-Strip level 0 of the multicolour smoother the launch is mc_strip_kernel, the count is its
 * colour stages and the bytes are row types + colours + x + f + out, f_H and the zeroed u_H.       */
amg_hip_status amg_hip_fine_sweep_info(const amg_hip_solver* s, char* name, int32_t name_cap,
                                       int32_t* sweeps_per_launch, double* bytes_per_launch);

/* ---- stand-alone plug-in operations on host arrays (run on the device) -----
 * SmootherBase::smooth(A, u, b), smoother.hpp:63-65, for the built-in kinds.
 * u is updated in place.  every = compute_error_every_n_iters (0 = never, the
 * SparseGaussSeidel() default); *iters and *converged mirror the reference's
 * loop (smoother.hpp:195-203).  For kinds 3-4 `n_iters` counts sweeps /
 * symmetric colour passes and tol/every are ignored.                          */
amg_hip_status amg_hip_smooth(int32_t kind, int64_t n, const int32_t* colptr,
                              const int32_t* rowind, const double* val,
                              double* u, const double* b, double omega,
                              double tol, int64_t every, int64_t n_iters,
                              int64_t* iters, int32_t* converged);
/* The Chebyshev smoother (AMG_HIP_SM_CHEBYSHEV) on host arrays: n_iters applications of the
 * degree-`degree` polynomial on [lower G, upper G], G the Gershgorin bound of D^-1 A computed
 * from the rows of A.  u is updated in place.  AMG_HIP_EINVAL: degree < 1, lower <= 0,
 * lower >= upper, n_iters < 0, or a zero diagonal.                                          */
amg_hip_status amg_hip_smooth_chebyshev(int64_t n, const int32_t* colptr, const int32_t* rowind,
                                        const double* val, double* u, const double* b,
                                        int32_t degree, double lower, double upper,
                                        int64_t n_iters);
/* The line smoother (AMG_HIP_SM_LINE_JACOBI) on host arrays: `iters` sweeps
 * u <- u + omega T^-1 (f - A u) with the lines at distance `stride`; stride = 0 takes the
 * automatic rule, any stride >= 1 is legal (every stride >= n means the same thing, each row
 * its own line, i.e. weighted Jacobi, and is taken as n).  u is updated in place.  AMG_HIP_EINVAL: stride < 0, iters < 0, omega
 * outside (0, 2), or a pivot of T that is zero or not finite (row in the message).         */
amg_hip_status amg_hip_smooth_line(int64_t n, const int32_t* colptr, const int32_t* rowind,
                                   const double* val, int64_t stride, double omega, int64_t iters,
                                   double* u, const double* f);
/* The alternating line smoother (AMG_HIP_SM_LINE_ALT) on host arrays: `iters` applications on the
 * dims[0] x dims[1] x dims[2] grid (dim 2 or 3, as amg_hip_create_tensor), directions ascending,
 * or descending with reverse = 1.  u is updated in place.  AMG_HIP_EINVAL: n != nx ny nz, a bad
 * dim or dims, omega outside (0, 2), iters < 0, or a bad pivot (direction and row in the message);
 * all of them are found before the device is touched.                                        */
amg_hip_status amg_hip_smooth_line_alt(int64_t n, const int32_t* colptr, const int32_t* rowind,
                                       const double* val, int32_t dim, const int64_t* dims, double omega,
                                       int64_t iters, int32_t reverse, double* u, const double* f);
/* amg_hip_smooth_line_alt with cyclic lines on the axes of `periodic_axes` (bit a = axis a) that
 * have 3 points or more ("cyclic lines" at amg_hip_create_tensor_periodic).  periodic_axes = 0 gives
 * amg_hip_smooth_line_alt bit for bit.  AMG_HIP_EINVAL: that function's checks, periodic_axes
 * negative or with bits at or above dim, a bad pivot of T' or T'^T or a bad denominator.       */
amg_hip_status amg_hip_smooth_line_alt_per(int64_t n, const int32_t* colptr, const int32_t* rowind,
                                           const double* val, int32_t dim, const int64_t* dims,
                                           int32_t periodic_axes, double omega, int64_t iters,
                                           int32_t reverse, double* u, const double* f);
/* One lexicographic sweep, dir=+1 forward (smoother.hpp:148-157) or -1 backward
 * (:167-174). */
amg_hip_status amg_hip_spgs_sweep(int32_t dir, int64_t n, const int32_t* colptr,
                                  const int32_t* rowind, const double* val,
                                  double* u, const double* b);
/* r = f - A*u, multigrid.hpp:272-274 (Eigen order: ascending column per row). */
amg_hip_status amg_hip_residual(int64_t n, const int32_t* colptr,
                                const int32_t* rowind, const double* val,
                                const double* u, const double* f, double* r);
/* out = M*v for a rows x cols CSC matrix: InterpolatorBase::prolongation /
 * restriction, interpolator.hpp:52-56,64-68. */
amg_hip_status amg_hip_spmv(int64_t rows, int64_t cols, const int32_t* colptr,
                            const int32_t* rowind, const double* val,
                            const double* v, double* out);
/* Built-in LinearInterpolator transfers without a matrix (bit-identical to
 * amg_hip_spmv on make_operators' P/R): f_H = R r  and  u_h += P u_H
 * (interpolator.hpp:106-141, multigrid.hpp:281-282,294-296). */
amg_hip_status amg_hip_linear_restrict(int64_t n_h, int64_t n_H, const double* r,
                                       double* f_H);
amg_hip_status amg_hip_linear_prolong_add(int64_t n_h, int64_t n_H,
                                          const double* u_H, double* u_h);
/* The transfers of amg_hip_create_tensor without a matrix, on host arrays: dims_h = the FINE grid
 * (3 entries, x fastest; dim = 2: dims_h[2] = 1), every coarsened axis at least 2 points, the
 * coarse grid floor(m / 2) per axis.  f_H = R r and u_h += P u_H, bit-identical to amg_hip_spmv
 * with the R / P that amg_hip_get_transfer returns: K-TensorRestrict adds the 9 (27) terms of a
 * coarse value in ascending fine index, K-TensorProlong the terms of a fine value in ascending
 * coarse index, and every weight product is exact.                                              */
amg_hip_status amg_hip_tensor_restrict(int32_t dim, const int64_t* dims_h /* 3 */, const double* r,
                                       double* f_H);
amg_hip_status amg_hip_tensor_prolong_add(int32_t dim, const int64_t* dims_h /* 3 */,
                                          const double* u_H, double* u_h);
/* The same two transfers with an axis mask (amg_hip_create_tensor_semi: bit 0 = x, 1 = y, 2 = z): a
 * masked axis needs 2 points and goes to floor(m / 2), an unmasked one keeps its length.  Still
 * bit-identical to amg_hip_spmv with the R / P of amg_hip_get_transfer.  AMG_HIP_EINVAL for a zero
 * mask, bit 2 when dim = 2, bits above 7 and a masked axis of fewer than 2 points.              */
amg_hip_status amg_hip_tensor_restrict_axes(int32_t dim, const int64_t* dims_h /* 3 */, int32_t axis_mask,
                                            const double* r, double* f_H);
amg_hip_status amg_hip_tensor_prolong_add_axes(int32_t dim, const int64_t* dims_h /* 3 */, int32_t axis_mask,
                                               const double* u_H, double* u_h);
/* K-AxisRestrict / K-AxisProlong on host arrays: one coarsened `axis` (0 = x, 1 = y, 2 = z; < dim, at
 * least 2 points) of the fine grid dims_h, with the compact weights W in the layout of
 * amg_hip_get_axis_weights (2 (n_h - n_H) doubles, any values).  f_H = R r and u_h += P u_H,
 * bit-identical to amg_hip_spmv with the R / P these weights stand for: every product is rounded
 * and the terms are added from +0.0 in ascending column order.                                   */
amg_hip_status amg_hip_axis_restrict(int32_t dim, const int64_t* dims_h /* 3 */, int32_t axis, const double* W,
                                     const double* r, double* f_H);
amg_hip_status amg_hip_axis_prolong_add(int32_t dim, const int64_t* dims_h /* 3 */, int32_t axis, const double* W,
                                        const double* u_H, double* u_h);
/* The same two transfers on an axis that wraps (periodic = 1: the PER forms of the kernels, the
 * weights and the column order of amg_hip_create_tensor_opdep_periodic; every pair of W holds two
 * weights, W[0] being w_lo of fine point 0 from the LAST coarse point).  Bit-identical to amg_hip_spmv
 * with the R / P these weights stand for.  periodic = 0: the pair above, same kernels, same bits.
 * AMG_HIP_EINVAL for periodic other than 0 / 1, and for periodic = 1 on an axis of odd length or of
 * fewer than 4 points.  vec_shift (0 or 1, else AMG_HIP_EINVAL): the device copies of the vectors
 * (not of W) start 8 * vec_shift bytes past a 16-byte boundary -- the load forms a caller with
 * unaligned vectors gets; the result does not depend on it.                                       */
amg_hip_status amg_hip_axis_restrict_per(int32_t dim, const int64_t* dims_h /* 3 */, int32_t axis, int32_t periodic,
                                         const double* W, const double* r, double* f_H, int32_t vec_shift);
amg_hip_status amg_hip_axis_prolong_add_per(int32_t dim, const int64_t* dims_h /* 3 */, int32_t axis,
                                            int32_t periodic, const double* W, const double* u_H, double* u_h,
                                            int32_t vec_shift);
/* The same two transfers with an axis mask and the side mask of opts->natural_sides (P1N on the
 * coarsened axes): bit-identical to amg_hip_spmv with the R / P of amg_hip_get_transfer of a solver
 * made with that side mask.  The argument checks of the _axes forms, plus AMG_HIP_EINVAL for a
 * negative `natural_sides` or bits at or above 2 dim.  natural_sides = 0: the _axes forms.        */
amg_hip_status amg_hip_tensor_restrict_bc(int32_t dim, const int64_t* dims_h /* 3 */, int32_t axis_mask,
                                          int32_t natural_sides, const double* r, double* f_H);
amg_hip_status amg_hip_tensor_prolong_add_bc(int32_t dim, const int64_t* dims_h /* 3 */, int32_t axis_mask,
                                             int32_t natural_sides, const double* u_H, double* u_h);
/* The same two transfers with an axis mask, a side mask and the periodic mask of
 * amg_hip_create_tensor_periodic (P1per on the coarsened periodic axes): bit-identical to
 * amg_hip_spmv with the R / P of amg_hip_get_transfer of such a solver.  The argument checks of the
 * _bc forms, plus AMG_HIP_EINVAL for `periodic_axes` negative or with bits at or above dim, a
 * coarsened periodic axis of odd length or fewer than 4 points, and a `natural_sides` bit on a
 * periodic axis.  periodic_axes = 0: the _bc forms, the same kernel and the same bits.            */
amg_hip_status amg_hip_tensor_restrict_per(int32_t dim, const int64_t* dims_h /* 3 */, int32_t axis_mask,
                                           int32_t natural_sides, int32_t periodic_axes, const double* r,
                                           double* f_H);
amg_hip_status amg_hip_tensor_prolong_add_per(int32_t dim, const int64_t* dims_h /* 3 */, int32_t axis_mask,
                                              int32_t natural_sides, int32_t periodic_axes, const double* u_H,
                                              double* u_h);
/* AMG::rss(A, u, b), common.hpp:17-27. */
amg_hip_status amg_hip_rss_host(int64_t n, const int32_t* colptr,
                                const int32_t* rowind, const double* val,
                                const double* u, const double* b, double* out);
/* x = A^-1 f by the banded LDL^T used for the coarsest level
 * (multigrid.hpp:287-288); *halfbw returns the bandwidth found. */
amg_hip_status amg_hip_coarse_solve(int64_t n, const int32_t* colptr,
                                    const int32_t* rowind, const double* val,
                                    const double* f, double* x, int64_t* halfbw);

/* The same solve by the partitioned (parallel) algorithm of opt.fast_coarse_solve. */
amg_hip_status amg_hip_coarse_solve_fast(int64_t n, const int32_t* colptr,
                                         const int32_t* rowind, const double* val,
                                         const double* f, double* x, int64_t* halfbw,
                                         int32_t* partition_rows);

/* ---- Grid<double> problem generators (grid.hpp), host side -----------------
 * laplacian: grid.hpp:88-98 (dim 2) / 7-point analogue (dim 3).  Call with NULL
 * arrays to get nnz.  rhs: grid.hpp:108-140, default Gaussian forcing.        */
int64_t amg_hip_laplacian(int32_t dim, int64_t n, int32_t* colptr,
                          int32_t* rowind, double* val);
amg_hip_status amg_hip_rhs(int32_t dim, int64_t n, double* b);

/* ---- device-pointer kernel launchers ----------------------------------------
 * For hosts that own device memory and streams themselves (the multi-GPU
 * row-block driver: torch tensors + torch.distributed halo exchange).  All
 * pointers are DEVICE pointers; `stream` is a hipStream_t (NULL = default).
 * CSR here = row-major view (rowptr/col/val); for a symmetric A the CSC arrays
 * are the CSR arrays.  Column indices address `u` directly, so a rank passes a
 * halo-extended local vector and locally renumbered columns.                  */
/* Host-only probe of the dictionary coding (no device needed): encodes the CSR block
 * the way amg_hip_devmat_create / the level upload would (exact zeros are NOT dropped
 * here), decodes it again and compares with the input.  AMG_HIP_OK: the block qualifies
 * and the round trip is exact; n_pairs = distinct (column offset, value) pairs,
 * n_row_types = distinct rows as whole code words (0 when more than 255, i.e. first
 * level only), words = 64-bit code words per row.  AMG_HIP_EUNSUPPORTED: it does not
 * qualify (more than 255 pairs, a row longer than 16 entries, ...).              */
amg_hip_status amg_hip_dict_probe(int64_t nrows, int64_t ncols, const int32_t* rowptr,
                                  const int32_t* col, const double* val, int64_t diag_shift,
                                  int32_t* n_pairs, int32_t* n_row_types, int32_t* words);
/* Launch parameters of the CSR kernels, computed from a HOST copy of rowptr:
 * max entries in any block of 256 consecutive rows, and the longest row.     */
amg_hip_status amg_hip_csr_shape(int64_t nrows, const int32_t* rowptr_host,
                                 int32_t* max_block_nnz, int32_t* max_row_nnz);
amg_hip_status amg_hip_dev_residual(int64_t nrows, int64_t nnz, int32_t max_block_nnz,
                                    int32_t max_row_nnz, const int32_t* rowptr,
                                    const int32_t* col, const double* val,
                                    const double* u, const double* f, double* r,
                                    void* stream);
/* u_out[i] = u_in[i'] + omega*((b[i]-sum_{j!=i'} a_ij u_in[j])/a_ii' - u_in[i'])
 * with i' = i + diag_shift: the column that is row i's diagonal (a rank passes
 * the offset of its first owned row inside its halo-extended vector). b and
 * u_out are indexed by the local row i.                                       */
amg_hip_status amg_hip_dev_jacobi(int64_t nrows, int64_t nnz, int32_t max_block_nnz,
                                  int32_t max_row_nnz, const int32_t* rowptr,
                                  const int32_t* col, const double* val,
                                  const double* u_in, const double* b,
                                  double* u_out, double omega, int64_t diag_shift,
                                  void* stream);
amg_hip_status amg_hip_dev_spmv(int64_t nrows, int64_t nnz, int32_t max_block_nnz,
                                int32_t max_row_nnz, const int32_t* rowptr,
                                const int32_t* col, const double* val,
                                const double* v, double* out, void* stream);
/* The same three operations on a matrix the LIBRARY uploads in its own device
 * layout (amg_hip_layout; AUTO = dictionary-coded when the block qualifies, else
 * SELL-64 panels; exact zeros dropped):
 * rows x cols local CSR block given on the host, columns indexing the vector the
 * operation is applied to.  op: 0 = residual (out = f - A x), 1 = Jacobi sweep
 * (diagonal of row i at column i + diag_shift), 2 = SpMV (f unused).  The
 * diag_shift given at creation (0 for a plain matrix) must be the one passed to
 * apply (the 16-bit relative column indices are built against it).            */
typedef struct amg_hip_devmat amg_hip_devmat;
amg_hip_status amg_hip_devmat_create(int64_t nrows, int64_t ncols, const int32_t* rowptr,
                                     const int32_t* col, const double* val, int32_t layout,
                                     int64_t diag_shift, int32_t device, amg_hip_devmat** out);
void amg_hip_devmat_destroy(amg_hip_devmat* m);
/* Layout the block was uploaded in and its matrix stream bytes (amg_hip_level_layout). */
amg_hip_status amg_hip_devmat_layout(const amg_hip_devmat* m, int32_t* layout,
                                     int64_t* matrix_stream_bytes);
amg_hip_status amg_hip_devmat_apply(const amg_hip_devmat* m, int32_t op, const double* x,
                                    const double* f, double* out, double omega,
                                    int64_t diag_shift, void* stream);
/* First Jacobi sweep from a zero vector: u_out[i] = 0 + omega*((b[i] - 0)/diag[i] - 0)
 * (diag[i] == 0 leaves 0); bit-identical to amg_hip_dev_jacobi on u_in == 0.   */
amg_hip_status amg_hip_dev_jacobi_from_zero(int64_t nrows, const double* diag,
                                            const double* b, double* u_out,
                                            double omega, void* stream);
/* y[i] += x[i] */
amg_hip_status amg_hip_dev_axpy1(int64_t n, const double* x, double* y, void* stream);
/* *out (device double) = sum_i r[i]^2 ; scratch >= 8 KiB device memory */
amg_hip_status amg_hip_dev_sumsq(int64_t n, const double* r, double* out,
                                 double* scratch, void* stream);

/* ---- peer-to-peer halo exchange over hipIpc (xGMI inside a node) --------------
 * The multi-GPU driver's neighbour exchange without a collective: every rank
 * allocates its exchangeable vectors inside one arena, exports it with hipIpc,
 * maps the arenas of rank-1 / rank+1, and then pushes its boundary unknowns
 * straight into the neighbour's halo slots with stream-ordered copies; arrival
 * and consumption are signalled with 32-bit epoch words in the arenas
 * (hipStreamWriteValue32 / hipStreamWaitValue32: no host synchronisation, no
 * spinning kernel).  Bootstrap (exchanging the 64-byte handles and the layout
 * tables) is done by the host through torch.distributed.                      */
typedef struct amg_hip_arena amg_hip_arena;
amg_hip_status amg_hip_arena_create(int64_t bytes, int32_t device, amg_hip_arena** out);
void amg_hip_arena_destroy(amg_hip_arena* a);
void* amg_hip_arena_base(const amg_hip_arena* a);
/* 64-byte hipIpcMemHandle_t of the arena */
amg_hip_status amg_hip_arena_export(const amg_hip_arena* a, uint8_t handle[64]);
amg_hip_status amg_hip_arena_open_peer(const uint8_t handle[64], void** peer_base);
amg_hip_status amg_hip_arena_close_peer(void* peer_base);

/* One exchange with both neighbours.  Any side may be absent (NULL / 0).
 * push_wait:  wait until the neighbours acknowledged epoch-1 (my previous data
 * has been consumed) -> copy my boundary into their halo slots -> publish
 * `epoch` in their arenas -> wait until their data of `epoch` has landed in
 * mine.  ack: tell the neighbours that the halo data of `epoch` has been
 * consumed (call it after the kernel that read the halos).                    */
typedef struct {
  void* dst_prev; const void* src_prev; int64_t bytes_prev;  /* my first rows -> rank-1's upper halo */
  void* dst_next; const void* src_next; int64_t bytes_next;  /* my last rows  -> rank+1's lower halo */
  uint32_t* data_flag_at_prev;  /* word in rank-1's arena: "data from my next has landed" */
  uint32_t* data_flag_at_next;  /* word in rank+1's arena: "data from my prev has landed" */
  uint32_t* my_data_from_prev;  /* words in MY arena the neighbours publish into          */
  uint32_t* my_data_from_next;
  uint32_t* ack_flag_at_prev;   /* word in rank-1's arena: "my next consumed my data"     */
  uint32_t* ack_flag_at_next;
  uint32_t* my_ack_from_prev;   /* words in MY arena: the neighbour consumed what I sent  */
  uint32_t* my_ack_from_next;
  uint32_t epoch;               /* 1, 2, 3, ... per channel                               */
  int32_t recv_from_prev;       /* 1 when rank-1 sends me data on this channel            */
  int32_t recv_from_next;
} amg_hip_halo_desc;
amg_hip_status amg_hip_halo_push_wait(const amg_hip_halo_desc* d, void* stream);
amg_hip_status amg_hip_halo_ack(const amg_hip_halo_desc* d, void* stream);

/* The same exchange as ONE graph-capturable kernel (no host-side stream memory
 * operations, which cost ~3 us each and cannot be captured): flags are 0/1 words
 * in the receiver's arena (DATA: "your halo slots hold my new values", FREE: "I
 * have consumed them"), accessed with system-scope atomics; spins are bounded
 * (~2 s) and report through *timeout (a device word the host can check).
 * FREE words must be initialised to 1 (amg_hip_fill_u32), DATA words to 0.      */
typedef struct {
  double* dst_prev; const double* src_prev; int64_t cnt_prev;   /* counts in doubles */
  double* dst_next; const double* src_next; int64_t cnt_next;
  uint32_t* my_free_from_prev; uint32_t* my_free_from_next;     /* in MY arena        */
  uint32_t* data_at_prev; uint32_t* data_at_next;               /* in the neighbours' */
  uint32_t* my_data_from_prev; uint32_t* my_data_from_next;     /* in MY arena        */
  int32_t recv_prev, recv_next;
  uint32_t* timeout;
} amg_hip_halo_kdesc;
amg_hip_status amg_hip_halo_exchange_kernel(const amg_hip_halo_kdesc* d, void* stream);
/* after the kernel that consumed the halos: FREE := 1 at the senders */
amg_hip_status amg_hip_halo_ack_kernel(uint32_t* free_at_prev, uint32_t* free_at_next,
                                       void* stream);
/* All-gather by direct pushes: my `cnt` doubles go to offset `off` of every rank's
 * full vector dst[g] (dst[rank] is my own); data_at[g] / free_at[g] are word [rank]
 * of rank g's DATA / FREE block, my_data_from / my_free_from my own blocks
 * (one word per rank).  world <= 16.                                          */
typedef struct {
  int32_t rank, world;
  const double* src; int64_t cnt, off;
  double* dst[16];
  uint32_t* data_at[16];
  uint32_t* free_at[16];
  uint32_t* my_data_from;
  uint32_t* my_free_from;
  uint32_t* timeout;
} amg_hip_gather_kdesc;
amg_hip_status amg_hip_gather_kernel(const amg_hip_gather_kdesc* d, void* stream);
amg_hip_status amg_hip_gather_ack_kernel(const amg_hip_gather_kdesc* d, void* stream);
amg_hip_status amg_hip_fill_u32(uint32_t* dev_ptr, int64_t count, uint32_t value, void* stream);

/* Stream capture helpers for hosts that drive the launchers above from another
 * language: everything enqueued on `stream` between begin and end becomes one
 * executable graph.                                                            */
amg_hip_status amg_hip_capture_begin(void* stream);
amg_hip_status amg_hip_capture_end(void* stream, void** graph_exec);
amg_hip_status amg_hip_graph_launch(void* graph_exec, void* stream);
void amg_hip_graph_destroy(void* graph_exec);

#ifdef __cplusplus
}
#endif
#endif /* AMG_HIP_H */
