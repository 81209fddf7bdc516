/*
 * nnpops_hip.h -- C ABI of libnnpops_hip.so, the MI355X (gfx950) implementation of the NNPOps
 * per-atom hot path: ANI symmetry functions, SchNet CFConv (+ neighbour list) and
 * getNeighborPairs.
 *
 * This is the drop-in boundary.  Every entry point replaces one method of the reference's
 * device-agnostic C++ core (the layer its torch binding calls into) or one torch dispatcher
 * kernel, and keeps that method's argument meaning:
 *
 *   nnpops_ani_create / _destroy     ANISymmetryFunctions ctor/dtor        src/ani/ANISymmetryFunctions.h:60-66
 *   nnpops_ani_set_stream            CudaANISymmetryFunctions::setStream   src/ani/CudaANISymmetryFunctions.h (setStream)
 *   nnpops_ani_compute               computeSymmetryFunctions              src/ani/ANISymmetryFunctions.h:78
 *   nnpops_ani_backprop              backprop                              src/ani/ANISymmetryFunctions.h:92
 *   nnpops_cfconv_neighbors_*        CFConvNeighbors ctor / build          src/schnet/CFConv.h:37-85
 *   nnpops_cfconv_create / compute / backprop   CFConv ctor / compute / backprop   src/schnet/CFConv.h:109-217
 *   nnpops_cfconv_backprop_box       (additive) backprop and the box-vector gradient of a periodic list
 *   nnpops_cfconv_double_backward    (additive) the backward of backprop: second derivatives w.r.t. positions and input
 *   nnpops_cfconv_double_backward_weights   (additive) the weight gradients of what double_backward differentiates (a force loss)
 *   nnpops_cfconv_backprop_weights / _set_weights   (additive) gradients of the filter network's four weight arrays; new weights for a
 *                                               live handle (trainable filters)
 *   nnpops_neighbor_pairs_forward / _backward   neighbors::getNeighborPairs forward/backward kernels
 *                                               src/pytorch/neighbors/getNeighborPairsCUDA.cu:31-101
 *   nnpops_neighbor_pairs_box_backward / _double_backward   box gradient and second derivatives of that op
 *                                               (the reference's CPU op differentiates both: getNeighborPairsCPU.cpp:56-98)
 *   nnpops_pme_direct                           pme::pme_direct (computeDirect)   src/pytorch/pme/pmeCUDA.cu:30-100
 *   nnpops_pme_direct_double_backward, nnpops_pme_reciprocal_spread_directional / _interpolate_second   second derivatives of both PME
 *                                               terms w.r.t. positions and charges (the reference refuses them)
 *   nnpops_pme_direct_box, nnpops_pme_reciprocal_convolve_box / _box_gradient   box gradients of both PME terms (no reference
 *                                               counterpart: pme::pme_direct_box and the box gradient of pme::pme_reciprocal)
 *
 * Conventions
 *   - plain C: opaque handles, raw pointers, sizes.  No torch / C++ types cross this boundary.
 *   - every pointer documented "device" is a HIP device pointer valid on the handle's device;
 *     "host" pointers are read during the call only.  float = IEEE fp32, indices = int32.
 *   - all work is enqueued on the handle's stream (default: the null stream); nothing
 *     synchronises the host unless the function says so.  Calls are graph-capturable unless noted.
 *   - every function returns 0 on success or a negative nnpops_status; nnpops_last_error()
 *     returns a thread-local message for the last failure.
 *   - a handle is not thread-safe and not re-entrant, like the reference's objects
 *     (backprop consumes state left by the last compute -- ANISymmetryFunctions.h:83-84).
 */
#ifndef NNPOPS_HIP_H
#define NNPOPS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    NNPOPS_OK = 0,
    NNPOPS_ERR_INVALID_ARGUMENT = -1,
    NNPOPS_ERR_HIP = -2,            /* a HIP runtime call failed; message carries hipGetErrorString */
    NNPOPS_ERR_UNSUPPORTED = -3,    /* configuration outside what the kernels were built for */
    NNPOPS_ERR_CAPACITY = -4,       /* a neighbour list outgrew its buffers (see *_check) */
    NNPOPS_ERR_NO_DEVICE = -5
} nnpops_status;

const char* nnpops_last_error(void);
/* Library / build identification: "nnpops_hip <version> gfx950". */
const char* nnpops_version(void);
/* Number of HIP devices visible; negative nnpops_status when the runtime is unusable. */
int nnpops_device_count(void);

/* ------------------------------------------------------------------------------------------
 * ANI symmetry functions (replaces ANISymmetryFunctions / CudaANISymmetryFunctions)
 * ------------------------------------------------------------------------------------------ */
typedef struct nnpops_ani* nnpops_ani_t;

/* radial_eta_rs:            host, [num_radial][2]   = {eta, rs}                 (RadialFunction,  ANISymmetryFunctions.h:29-32)
 * angular_eta_rs_zeta_ths:  host, [num_angular][4]  = {eta, rs, zeta, thetas}   (AngularFunction, ANISymmetryFunctions.h:34-39)
 * atom_species:             host, [num_atoms], values in [0, num_species)
 * periodic / torchani:      as the reference constructor flags
 * device:                   HIP device ordinal the handle lives on
 * Any list of angular functions is accepted, like the reference core (CpuANISymmetryFunctions.cpp:153-194).  A list that
 * is a full grid {(eta,rs)} x {(zeta,thetas)} of at most 16 x 8 distinct factors -- every set the reference's torch binding
 * can build (SymmetryFunctions.cpp:115-120), ANI-1x/1ccx/2x included -- runs on the factored matrix-core kernels; any other
 * list runs on generic kernels (same results, several times slower). */
int nnpops_ani_create(nnpops_ani_t* out, int num_atoms, int num_species, float radial_cutoff, float angular_cutoff,
                      int periodic, const int32_t* atom_species, int num_radial, const float* radial_eta_rs,
                      int num_angular, const float* angular_eta_rs_zeta_ths, int torchani, int device);
int nnpops_ani_destroy(nnpops_ani_t h);
/* stream: a hipStream_t passed as void* (NULL = null stream). */
int nnpops_ani_set_stream(nnpops_ani_t h, void* stream);

/* positions: device [num_atoms][3]; box: device [3][3] rows = box vectors (ignored, may be NULL,
 * when the handle is not periodic); radial: device [num_atoms][num_species][num_radial];
 * angular: device [num_atoms][num_species*(num_species+1)/2][num_angular].  Outputs are fully
 * overwritten.  Positions / box / neighbour lists are retained for backprop.
 * A periodic handle with molecules (nnpops_ani_set_molecules): box is device [num_molecules][3][3], molecule m uses rows
 * 9m .. 9m+8 and wraps the displacements among its own atoms in it. */
int nnpops_ani_compute(nnpops_ani_t h, const float* positions, const float* box, float* radial, float* angular);
/* radial_deriv / angular_deriv: device, shapes as the outputs above; position_deriv: device
 * [num_atoms][3], fully overwritten.  Must follow a compute() on the same handle. */
int nnpops_ani_backprop(nnpops_ani_t h, const float* radial_deriv, const float* angular_deriv, float* position_deriv);
/* The same two calls for AEV / gradient arrays whose rows are embedded in wider rows: row i of the radial part
 * starts at radial + i * radial_ld (floats), likewise angular; 0 = dense.  Lets a caller keep ONE [num_atoms][W_r + W_a]
 * array (radial = aev, angular = aev + W_r, both strides W_r + W_a) -- the layout TorchANI's AEVComputer returns --
 * without a concatenation copy forward and a split copy backward. */
int nnpops_ani_compute_strided(nnpops_ani_t h, const float* positions, const float* box, float* radial, int radial_ld,
                               float* angular, int angular_ld);
int nnpops_ani_backprop_strided(nnpops_ani_t h, const float* radial_deriv, int radial_ld, const float* angular_deriv,
                                int angular_ld, float* position_deriv);
/* backprop_strided followed by the box-vector gradient (virial) of the same scalar L = sum radial_deriv * radial + sum angular_deriv *
 * angular.  Every displacement of the AEV is d = x_j - x_i + n B with B = box (rows = vectors) and n the integer minimum-image shift
 * compute() chose, held fixed: box_deriv[k][c] = sum over every use of a displacement of n_k (dL/dd)_c -- all nine entries, the same
 * formal derivative as nnpops_neighbor_pairs_box_backward.  box_deriv: device [3][3], fully overwritten (float32, accumulated in
 * float64 in a fixed order: two calls agree bit for bit); position_deriv is exactly what backprop_strided writes.
 * CONTRACT: positions and box are the arrays of the preceding compute(), unchanged -- the shifts are recovered from them and from
 * the displacements the handle kept, not stored.  Periodic handles only (NNPOPS_ERR_INVALID_ARGUMENT otherwise, with or without
 * molecules).
 * A periodic handle with molecules (a periodic batch, nnpops_ani_set_molecules): box and box_deriv are device [num_molecules][3][3];
 * molecule m's nine entries are the same sum over the displacements of ITS atoms only, shifts recovered against box m.  A number of
 * workgroups per molecule that depends on its atom count alone, then one sum per molecule: float64, a fixed order, no atomics, the
 * partial sums in a workspace nnpops_ani_set_molecules sized: two calls agree bit for bit and
 * a molecule's entries do not depend on its companions.  position_deriv is again exactly what backprop_strided writes.
 * Allocates nothing: graph-capturable like backprop.  Additive. */
int nnpops_ani_backprop_box_strided(nnpops_ani_t h, const float* positions, const float* box, const float* radial_deriv, int radial_ld,
                                    const float* angular_deriv, int angular_ld, float* position_deriv, float* box_deriv);
/* The tangent J.v of the AEV: the directional derivative d/dt aev(x + t v) at t = 0 along position_tangent (device [num_atoms][3]), on
 * the lists the preceding compute() left (shifts and box held fixed: the tangent of every displacement is v_j - v_i, so periodic
 * handles, non-periodic ones and nnpops_ani_set_molecules batches are alike).  What the parameter gradient of a force loss needs of the
 * AEV: with F = -J^T g(theta, aev) it is (dg/dtheta)^T (J.v), v = dL/dF.  It is the adjoint of backprop:
 * <w, tangent(v)> = <backprop(w), v>.  radial_tangent / angular_tangent: shapes and strides as compute_strided (0 = dense), fully
 * overwritten, zeros for atoms without neighbours.  One owner per element, no atomics: two calls agree bit for bit.  Any function
 * list (factorable or generic), both angle conventions.  Reads what compute() left and writes only its outputs: compute, backprop and
 * backprop_box around it keep their bits.  Allocates nothing, honours the handle's stream: graph-capturable like backprop.  Additive.
 * Second derivatives of the AEV in the positions or the box (Hessians, a force loss differentiated in the coordinates) are NOT here. */
int nnpops_ani_tangent_strided(nnpops_ani_t h, const float* position_tangent, float* radial_tangent, int radial_ld,
                               float* angular_tangent, int angular_ld);
/* Blocks on the handle's stream and reports whether the last compute() overflowed a neighbour
 * buffer (NNPOPS_ERR_CAPACITY; the handle has then already grown its buffers, so simply call
 * compute() again).  max_radial_neighbors / max_angular_neighbors (host, may be NULL) receive the
 * largest per-atom counts seen.  Not graph-capturable.
 * The first clean check() fits the row capacity to the system (longest row + 25 % + 8, NNPOPS_ERR_CAPACITY once: call
 * compute() again).  A caller that then stops checking -- a captured graph replayed for many steps -- relies on that
 * slack: a row that outgrows it is clamped (the builders raise a device-side flag that only check() reads), so call
 * check() every few hundred replays, or after anything that can change the density. */
int nnpops_ani_check(nnpops_ani_t h, int* max_radial_neighbors, int* max_angular_neighbors);
/* The device-side flag itself: *word receives the DEVICE address of one int32 that the neighbour builders OR into whenever a
 * compute() overflows a capacity (bit 0 rows / records, bit 1 box too small for the cell stencil, bit 2 cell bins, bit 3 an
 * atom outgrew the class of its backward launch) and that only nnpops_ani_check() clears.  It is STICKY: a captured graph
 * that is replayed without any check leaves its overflows there, so a caller can (a) put its own 4-byte asynchronous copy of
 * the word into the graph, or read it every N replays, without calling into this library, and (b) rely on the next eager
 * check() -- any later compute() followed by check() -- to report NNPOPS_ERR_CAPACITY for what happened during the replays:
 * a non-zero word found there means that every evaluation since the previous check may have been incomplete.  The address is
 * valid for the life of the handle. */
int nnpops_ani_overflow_word(nnpops_ani_t h, const int32_t** word);
/* The same word read for the caller: waits for the handle's stream, copies the four bytes with THIS library's HIP runtime (a host
 * layer that opens a HIP runtime of its own to copy from the address above may get a second runtime that does not know the
 * pointer) and leaves the word as it is -- only nnpops_ani_check() clears it.  Additive. */
int nnpops_ani_read_overflow(nnpops_ani_t h, int32_t* value);
/* The cell grid the last compute() decided on the device, for diagnostics and tests: waits for the handle's stream and copies it
 * with this library's runtime as out = {nx, ny, nz, ncells, m, ok, bin_overflow, periodic} (m: stencil half-width in cells, 1 for
 * cells at least a cutoff wide, 2 for half-width cells; ok = 0: the box was refused, or a bin overflowed, and check() falls back
 * or grows).  What it returns before any compute() went through the grid is unspecified; after a fall-back to the all-pairs search
 * it stays what the refused build left.  Blocks, runs no kernel, not capturable into a graph.  Additive. */
int nnpops_ani_read_grid(nnpops_ani_t h, int32_t* out);
/* Which kernels this handle runs, as one line of `key=value` words (for logs and tests; the words may grow): forward= merge |
 * chunked | mfma; backward= kernel number; generic= the function list does not factor; uniform= one eta and one zeta; grid= eight
 * radial factors on equally spaced shifts (taken by recurrence); literal= the constants are the published ANI-2x set and the
 * forward kernels carry them as literals; dynamic_quads, fused_build, cap, cap_angular, chunk, classes, cells: state after the last
 * compute() / check().  A periodic handle with molecules appends batch_boxes=1 (the builder with one box per molecule runs); on every
 * other handle the word is absent.  What the last backprop() launched (host-side records, no device work): bwd_mode= 0 the first-generation
 * angular backward (what runs when the pair matrix of the records does not fit the LDS, or on request), 1-4 the pair-matrix
 * kernels (1 / 3 one / two waves per atom with 16-byte gradient loads, 2 / 4 the same with the gradient row staged in LDS; where
 * the launch ran by class, the top class's mode); radial_bwd= lanes | rows (a lane per neighbour, or the first-generation row
 * kernel); tile= and compact= the pair-matrix edge and the compact-layout flag mode 0 was launched with (-1 when it did not run).
 * Before any backprop(): bwd_mode=-1 radial_bwd=none tile=-1 compact=-1.  The line stays below 512 bytes.
 * Writes at most `capacity` bytes including the terminator.  Additive. */
int nnpops_ani_describe(nnpops_ani_t h, char* text, int capacity);
/* The same check in two halves for callers that have more work to queue behind compute(): _begin (right after compute) queues
 * one single-thread launch that publishes the overflow word and a stamp into pinned host memory and returns 1 -- or 0 when the check cannot be deferred (first calls, while
 * capacities are still being fitted): call nnpops_ani_check() then.  _end (after the consumers of this build have been launched;
 * they clamp their counts, so an overflowed build is incomplete but harmless to run) polls that stamp (no API call) and returns what
 * nnpops_ani_check() would: NNPOPS_OK, or NNPOPS_ERR_CAPACITY after growing the buffers -- compute() and everything queued
 * behind it must then be issued again.  Additive (the reference has no capacity check: its neighbour list is the N x N matrix). */
int nnpops_ani_check_begin(nnpops_ani_t h);
/* _begin without its launch, for a caller whose NEXT kernel on the stream can do the publishing itself (nnpops_mlp_forward with
 * the frame's publish_* fields): returns 1 and the three values to hand to that kernel, or 0 when the check cannot be deferred.
 * The caller must launch that kernel before nnpops_ani_check_end(), which otherwise waits for the stream and runs the full check. */
int nnpops_ani_check_begin_with(nnpops_ani_t h, const int32_t** word, int32_t** publish_to, int32_t* stamp);
int nnpops_ani_check_end(nnpops_ani_t h);
/* Neighbour search used by compute(): 0 = automatic, 1 = all-pairs scan (the reference's
 * algorithm, O(N^2)), 2 = cell list (O(N); periodic boxes must be at least 3 cells wide per axis). */
int nnpops_ani_set_neighbor_algorithm(nnpops_ani_t h, int algorithm);
/* Which launches build the cell grid of a periodic system of up to 20 000 atoms: 1 (default; $NNPOPS_ANI_GRID_OWNED=0 at
 * create: 0) one launch in which every block orders the cells it owns, 0 the two launches bin_atoms + order_binned.  Results
 * are bit-identical; a handle may change from call to call (tests, A/B measurements).  describe() of a handle whose search
 * goes through the cell grid: grid_build=owned|binned (scan: the five-launch build of non-periodic and larger systems). */
int nnpops_ani_set_grid_build(nnpops_ani_t h, int one_launch);

/* Batched evaluation of independent molecules (or periodic frames) in one handle (the reference has no batch
 * dimension: src/pytorch/SymmetryFunctions.py:110; this is the additive API SURVEY.md s8f ranks second).
 * Atoms [molecule_offsets[m], molecule_offsets[m+1]) form molecule m (host array, num_molecules+1 entries,
 * first 0, last num_atoms); atoms of different molecules never see each other.  compute()/backprop() are
 * unchanged -- every kernel is per atom -- so one launch sequence evaluates the whole batch.
 * On a PERIODIC handle every molecule is a frame in a box of its own: the box of compute() / backprop_box is then a device
 * array [num_molecules][3][3] (molecule m: rows 9m .. 9m+8), and the atoms of molecule m see each other through the minimum
 * image of box m -- the single-round rule of a single frame (z, then y, then x, each by the diagonal entry).  As for a single
 * frame every box must be at least two radial cutoffs wide; that is the caller's contract and is not checked on the device.
 * The neighbour search of a batch is the all-pairs scan inside the molecule (never the cell grid): meant for frames of tens to
 * a few hundred atoms -- a 64-water box -- not for frames of thousands.
 * num_molecules <= 0 restores the single-system behaviour (a periodic handle: one [3][3] box again). */
int nnpops_ani_set_molecules(nnpops_ani_t h, int num_molecules, const int32_t* molecule_offsets);

/* Per-kernel timing with HIP events recorded on the handle's stream around kernel launches
 * (off by default; not for use during graph capture).  enable: 0 = off, 1 = every kernel, any other
 * value = a mask with bit (id + 1) set for each kernel id to time (an event pair costs ~3 us of stream
 * time on MI355X, so a benchmark times only the kernel it reports on).  get_timing blocks on the
 * stream, returns for each kernel id the summed duration in milliseconds and the number of launches
 * since the last call / enable, and resets the counters.  Arrays have NNPOPS_ANI_NUM_KERNELS entries. */
enum {
    NNPOPS_ANI_K_NEIGHBORS = 0,       /* neighbour rows + records + triple lists + radial AEV (one launch) */
    NNPOPS_ANI_K_RADIAL_FWD = 1,      /* always 0 launches: the radial AEV is written by the neighbour kernel */
    NNPOPS_ANI_K_ANGULAR_FWD = 2,     /* 0 launches for small systems: build + radial + angular forward are one kernel there, timed as NEIGHBORS */
    NNPOPS_ANI_K_RADIAL_BWD = 3,
    NNPOPS_ANI_K_ANGULAR_BWD = 4,
    NNPOPS_ANI_K_CELL_GRID = 5,       /* the grid build in front of the neighbour kernel (2 or 5 launches; 0 for all-pairs) */
    NNPOPS_ANI_NUM_KERNELS = 6
};
int nnpops_ani_enable_timing(nnpops_ani_t h, int enable);
/* Bracket only every `every`-th launch of each selected kernel (default 1 = every launch): a benchmark that must
 * measure its kernel inside the timed region pays the ~3 us per event that way on a sample of the steps only. */
int nnpops_ani_set_timing_stride(nnpops_ani_t h, int every);
int nnpops_ani_get_timing(nnpops_ani_t h, double* total_ms, int* launches);
/* What an event pair reports for an EMPTY bracket on the handle's stream (median of 21, milliseconds; blocks):
 * subtract it from a per-launch average to compare with a profiler's kernel durations. */
int nnpops_ani_timing_overhead(nnpops_ani_t h, double* ms);
/* merge != 0: while timing is enabled there is ONE bracket around neighbour build + angular forward (its time is reported under the
 * neighbour build) and ONE around angular backward + radial backward (reported under the angular backward); the four single
 * brackets are off, the cell grid's stays.  (single bracket A) + (single bracket B) - (merged bracket A+B) is what ONE bracket adds
 * to the stream -- measured in place, same launches, same cache state -- which is how bench.py makes its event figures comparable
 * with rocprofv3's kernel durations.  merge = 0 restores the per-kernel brackets.  Nothing changes when timing is off. */
int nnpops_ani_set_timing_merge(nnpops_ani_t h, int merge);

/* ------------------------------------------------------------------------------------------
 * SchNet continuous-filter convolution (replaces CFConvNeighbors / CFConv and their Cuda* subclasses)
 * ------------------------------------------------------------------------------------------ */
typedef struct nnpops_cfconv_neighbors* nnpops_cfconv_neighbors_t;
typedef struct nnpops_cfconv* nnpops_cfconv_t;

int nnpops_cfconv_neighbors_create(nnpops_cfconv_neighbors_t* out, int num_atoms, float cutoff, int periodic, int device);
int nnpops_cfconv_neighbors_destroy(nnpops_cfconv_neighbors_t h);
int nnpops_cfconv_neighbors_set_stream(nnpops_cfconv_neighbors_t h, void* stream);
/* positions: device [num_atoms][3]; box: device [3][3] or NULL.  Builds the half list
 * {(i,j): j>i, r_ij^2 < cutoff^2} with stored distances (CFConv.h:57, CpuCFConv.cpp:104-115). */
int nnpops_cfconv_neighbors_build(nnpops_cfconv_neighbors_t h, const float* positions, const float* box);
/* Blocks; num_pairs (host) receives the number of half pairs of the last build;
 * NNPOPS_ERR_CAPACITY if that build overflowed (buffers already grown: build again). */
int nnpops_cfconv_neighbors_check(nnpops_cfconv_neighbors_t h, int* num_pairs);
/* Blocks; copies the half list of the last build to host arrays (test/diagnostic use):
 * pair_atoms [2][capacity] (row 0 = i, row 1 = j), distances [capacity]. */
int nnpops_cfconv_neighbors_export(nnpops_cfconv_neighbors_t h, int capacity, int32_t* pair_atoms, float* distances);
/* The cell grid of the last build() that went through one (1 024 atoms and more), as nnpops_ani_read_grid:
 * out = {nx, ny, nz, ncells, m, ok, bin_overflow, periodic}.  Blocks, runs no kernel, not capturable; diagnostics only. */
int nnpops_cfconv_neighbors_read_grid(nnpops_cfconv_neighbors_t h, int32_t* out);

/* activation: 0 = shifted softplus, 1 = tanh (CFConv.h:114-117).
 * w1: host [width][num_gaussians] (the layout the reference core indexes, CpuCFConv.cpp:163);
 * b1: host [width]; w2: host [width][width] ([out][in]); b2: host [width]. */
int nnpops_cfconv_create(nnpops_cfconv_t* out, int num_atoms, int width, int num_gaussians, float cutoff, int periodic,
                         float gaussian_width, int activation, const float* w1, const float* b1, const float* w2,
                         const float* b2, int device);
int nnpops_cfconv_destroy(nnpops_cfconv_t h);
int nnpops_cfconv_set_stream(nnpops_cfconv_t h, void* stream);
/* input / output: device [num_atoms][width]; output fully overwritten (CFConv.h:169-171).
 * Widths 16, 32, ... 128 evaluate the filter network once per pair and keep one filter row per pair in a
 * scratch buffer owned by the convolution (num_atoms * row capacity / 2 rows of `width` floats; 164 MB for 10 000
 * atoms at width 128): it is allocated by the first compute()/backprop() with a given neighbour list, so run one
 * step before capturing a HIP graph.  For widths 32, 64, 96, 128 the dense layers are evaluated as split-fp16
 * matrix products with fp32 accumulation (every fp32 operand = two fp16 planes, 22 significant bits; at least as
 * accurate as a chain of fp32 FMAs) whenever the weights keep all operands inside the fp16 range; otherwise, or with
 * NNPOPS_CFCONV_SPLIT=0 in the environment at creation, on the fp32 matrix instruction. */
int nnpops_cfconv_compute(nnpops_cfconv_t h, nnpops_cfconv_neighbors_t neighbors, const float* positions,
                          const float* box, const float* input, float* output);
/* output_deriv: device [num_atoms][width]; input_deriv: device [num_atoms][width];
 * position_deriv: device [num_atoms][3]; both fully overwritten (CFConv.h:186-189). */
int nnpops_cfconv_backprop(nnpops_cfconv_t h, nnpops_cfconv_neighbors_t neighbors, const float* positions,
                           const float* box, const float* input, const float* output_deriv, float* input_deriv,
                           float* position_deriv);
/* As nnpops_cfconv_backprop, and the box-vector gradient (virial) of a periodic list behind it:
 *     box_deriv[k][c] = sum over the half pairs i < j of  n_ij,k * (dL/dd_ij)_c ,   d_ij = x_j - x_i + n_ij * box
 * with the minimum-image shifts n_ij the neighbour build chose held fixed; all nine entries, upper triangle included.
 * box_deriv: device float32 [3][3], fully overwritten (products and sums in float64, no atomics: two calls agree bit for bit).
 * positions and box are REQUIRED here and must be those of the neighbour list's last build(): the shifts are recovered from them
 * and the stored displacements.  A non-periodic list or a NULL pointer is an error.  input_deriv and position_deriv are what
 * nnpops_cfconv_backprop gives in the same place, bit for bit.  Runs on the convolution's stream; its scratch (partial sums; for
 * the vector kernels one float per neighbour-row entry) is allocated by the first call with a given list, so run one step before
 * capturing a HIP graph.  The stress follows as (sum_i x_i (x) dL/dx_i + box^T box_deriv) / V. */
int nnpops_cfconv_backprop_box(nnpops_cfconv_t h, nnpops_cfconv_neighbors_t neighbors, const float* positions,
                               const float* box, const float* input, const float* output_deriv, float* input_deriv,
                               float* position_deriv, float* box_deriv);
/* The backward of nnpops_cfconv_backprop (second derivatives for training on forces and Hessian-vector products).  backprop maps
 * (output_deriv g, input x, positions) to input_deriv gx and position_deriv gp; with cotangents gg_input_deriv V [N][W] of gx and
 * gg_position_deriv Q [N][3] of gp this returns the gradients of M = <V, gx> + <Q, gp>:
 *     out_output_deriv [N][W] = dM/dg,   out_input [N][W] = dM/dx,   out_positions [N][3] = dM/dpositions
 * with the pair set and the minimum-image shifts of the list's last build() held fixed (no gradient flows into the list, none into
 * the box; the filter network's weights are constants).  Either cotangent may be NULL, meaning zero, but not both.  The three outputs
 * are fully overwritten.  One owner-computes kernel over the neighbour rows: no atomics (two calls agree bit for bit), no scratch, no
 * allocation and no host synchronisation, so it can be captured into a HIP graph; it runs on the convolution's stream and leaves what
 * compute / backprop keep between calls untouched.  positions is not read (the list stores the displacements of its build). */
int nnpops_cfconv_double_backward(nnpops_cfconv_t h, nnpops_cfconv_neighbors_t neighbors, const float* positions, const float* input,
                                  const float* output_deriv, const float* gg_input_deriv, const float* gg_position_deriv,
                                  float* out_output_deriv, float* out_input, float* out_positions);
/* The number of the list's last build (a process-wide counter, never 0 for a built list; 0 before the first build): what was
 * computed for one build of a list may be told apart from a later one. */
int nnpops_cfconv_neighbors_build_count(nnpops_cfconv_neighbors_t h, unsigned long long* count);
/* Batched evaluation of independent NON-PERIODIC molecules behind one list (the counterpart of nnpops_ani_set_molecules, same
 * convention): atoms [molecule_offsets[m], molecule_offsets[m+1]) form molecule m (host array, num_molecules + 1 entries, first 0, last
 * num_atoms, strictly increasing); atoms of different molecules never become neighbours, however their coordinates overlap.  The
 * per-atom segment table is uploaded here, once; build() then fills the rows with a scan of every atom's own molecule (all pairs inside
 * the segment at every total size -- a shared cell grid says nothing about overlapping molecules -- so a molecule of many hundreds of
 * atoms costs its square), in ascending index order: a molecule's rows, pair slots and summation order are those of a list that holds
 * the molecule alone.  check(), capacity growth, export(), build_count() and nnpops_cfconv_compute / _backprop / _double_backward work
 * as they are: one launch sequence evaluates the whole batch.  Refused: a periodic list, offsets that do not start at 0 or end at
 * num_atoms, an empty or decreasing segment; build() with a box on such a list is an error, and nnpops_cfconv_backprop_box refuses it as
 * any non-periodic list.  The current build is invalidated (build_count() returns 0 until the next build()).  num_molecules <= 0 (or a
 * NULL table) restores the single-system list.  Blocks on the list's stream; not capturable. */
int nnpops_cfconv_neighbors_set_molecules(nnpops_cfconv_neighbors_t h, int num_molecules, const int32_t* molecule_offsets);
/* Batched evaluation of PERIODIC frames behind one list, every frame in its own box (a minibatch of an NPT trajectory): atoms
 * [frame_offsets[m], frame_offsets[m+1]) form frame m (host array, num_frames + 1 entries, first 0, last num_atoms, strictly
 * increasing).  Valid on a list created periodic = 1 only.  With frames set
 *   - nnpops_cfconv_neighbors_build reads box as device [num_frames][3][3]: atom i of frame m is paired only with atoms of its own
 *     frame, through the minimum image of box[m] (the single-round rule of a single system; every box at least two cutoffs wide, the
 *     caller's contract).  Frames are scanned all-pairs at every total size, candidates in ascending index order: a frame's rows, pair
 *     slots and summation order are those of a periodic list that holds the frame alone;
 *   - nnpops_cfconv_backprop_box reads box as [num_frames][3][3] and writes box_deriv [num_frames][3][3]: frame m's nine entries are
 *     summed over its own pairs, shifts recovered against box[m], in float64 in a fixed order that depends on the frame's atom count
 *     alone (no atomics: two calls agree bit for bit, and a frame's entries do not depend on its companions or its place);
 *   - every other entry point is unchanged: check(), capacity growth, export(), nnpops_cfconv_compute / _backprop / _double_backward /
 *     _backprop_weights / _double_backward_weights work from the stored rows.
 * Every table is sized and uploaded by this call, those of the box pass included, so build, compute, backprop and backprop_box stay
 * capturable once the row capacity has settled (the partial sums of the box pass belong to the convolution and are sized by its
 * first nnpops_cfconv_backprop_box on a list of frames, as its other scratch).  Refused: a non-periodic list, offsets that do not start
 * at 0 or end at num_atoms, an empty or decreasing frame; build() without a box on such a list is an error.  The current build is
 * invalidated.  num_frames <= 0 (or a NULL table) restores the single-system list.  Blocks on the list's stream; not capturable. */
int nnpops_cfconv_neighbors_set_frames(nnpops_cfconv_neighbors_t h, int num_frames, const int32_t* frame_offsets);
/* The plan of a convolution: which kernels a layer of this shape and these weights runs, and how they are launched.  Pure host
 * arithmetic (no device is needed or touched); it reads the NNPOPS_CFCONV_* switches as nnpops_cfconv_create does and refuses what
 * create refuses about the layer (NULL weights, activation, gaussian_width, num_gaussians, width).  w1, b1, w2 as for create.
 *     out[0]  path: 0 vector kernel, 1 filters on the fp32 matrix instruction, 2 split-fp16 filters through LDS planes,
 *             3 split-fp16 filters fed from registers (1-3: followed by the owner-computes gather, which takes no dynamic LDS)
 *     out[1]  waves per workgroup of the forward launch (vector kernel or filters kernel)
 *     out[2]  its dynamic LDS in bytes
 *     out[3]  waves per workgroup of the backward launch
 *     out[4]  its dynamic LDS in bytes
 *     out[5]  vector path: channels per lane (1, 2, 4 or 8; the same in both directions); else 0
 *     out[6]  vector path: bit 0 = the forward launch keeps its weights in LDS, bit 1 = the backward launch does (a clear bit:
 *             streamed through the caches); else 0
 *     out[7]  log2 of the power of two the split-fp16 backward kernels scale dY1 by (0 where the width has no split kernels) */
int nnpops_cfconv_plan(int width, int num_gaussians, float gaussian_width, int activation, const float* w1, const float* b1,
                       const float* w2, int32_t out[8]);
/* The same eight words for a handle: what its compute() and backprop() launches use (they go through the same arithmetic). */
int nnpops_cfconv_describe(nnpops_cfconv_t h, int32_t out[8]);
/* The gradients of a scalar L with respect to the filter network's four weight arrays, given output_deriv = dL/doutput [N][W] of
 * nnpops_cfconv_compute on the list's last build():
 *     w1_deriv [W][G],   b1_deriv [W],   w2_deriv [W][W] ([out][in]),   b2_deriv [W]       (the layouts create() takes)
 * All pointers are device pointers and none may be NULL; the four outputs are fully overwritten.  Only the list's stored distances,
 * input and output_deriv are read, so periodic and batched lists work as they are.  First derivatives only: nothing here is
 * differentiated further.  One kernel over the pair slots (the fp32 matrix instruction where the width is a multiple of 16 up to 128
 * and the weights fit in LDS, a vector kernel otherwise, whatever path the forward runs) writes one partial row per workgroup, a
 * second adds the rows in a fixed order in float64: no atomics, two calls agree bit for bit, a list without pairs gives exact
 * zeros.  Runs on the convolution's stream with no host synchronisation; its scratch (the partial rows, at most 32 MiB) is allocated by
 * the first call and sized once, so run one step before capturing a HIP graph.  What compute / backprop keep between calls (the
 * filter rows) is left untouched. */
int nnpops_cfconv_backprop_weights(nnpops_cfconv_t h, nnpops_cfconv_neighbors_t neighbors, const float* input, const float* output_deriv,
                                   float* w1_deriv, float* b1_deriv, float* w2_deriv, float* b2_deriv);
/* The weight gradients of a force loss: the gradients, with respect to the filter network's four weight arrays, of the scalar that
 * nnpops_cfconv_double_backward differentiates.  With output_deriv g, input x and the cotangents gg_input_deriv V [N][W] of backprop's
 * input_deriv and gg_position_deriv Q [N][3] of its position_deriv, M = <V, gx> + <Q, gp>, and this returns
 *     w1_deriv [W][G] = dM/dw1,   b1_deriv [W],   w2_deriv [W][W] ([out][in]),   b2_deriv [W]       (the layouts create() takes)
 * for the list's last build(), the pair set and the minimum-image shifts held fixed.  Either cotangent may be NULL, meaning zero, but
 * not both; with Q NULL the result is that of nnpops_cfconv_backprop_weights with V in the place of input.  All pointers are device
 * pointers; the four outputs are fully overwritten.  Only the list's rows, stored distances and pair slots and the per-atom arrays are
 * read, so periodic and batched lists work as they are.  Nothing here is differentiated further (no weight-weight second
 * derivatives).  With Q given, a short pass over the neighbour rows first writes the pair scalar u.(Q_j - Q_i) per pair slot; one kernel
 * over the pair slots (the fp32 matrix instruction where the width is a multiple of 16 up to 128 and its LDS image -- both weight
 * matrices, six pair tiles and two Gaussian tiles -- fits in 160 KiB, a vector kernel otherwise) then writes one partial row per
 * workgroup, and nnpops_cfconv_backprop_weights' finish adds the rows in a fixed order in float64: no atomics, two calls agree bit
 * for bit, a list without pairs gives exact zeros.  Runs on the convolution's stream with no host synchronisation; its scratch (one
 * float per pair slot, and the partial rows it shares with nnpops_cfconv_backprop_weights, at most 32 MiB) is allocated by the first call
 * and again only when the list's capacity has grown, so run one step before capturing a HIP graph.  What compute / backprop keep
 * between calls (the filter rows) is left untouched. */
int nnpops_cfconv_double_backward_weights(nnpops_cfconv_t h, nnpops_cfconv_neighbors_t neighbors, const float* input,
                                          const float* output_deriv, const float* gg_input_deriv, const float* gg_position_deriv,
                                          float* w1_deriv, float* b1_deriv, float* w2_deriv, float* b2_deriv);
/* New weights for a live convolution (after an optimizer step): four HOST arrays exactly as nnpops_cfconv_create takes them.  The plan
 * is made again from the new values (the split-fp16 decision and word 7 depend on them; nnpops_cfconv_describe reports the new plan),
 * every packed form create() uploads is uploaded again and the kept filter rows are forgotten: the handle then computes, bit for
 * bit, what a fresh handle created with these weights computes.  It waits for the handle's stream and copies synchronously: it blocks
 * and cannot be captured into a HIP graph (a captured graph of this handle keeps launching the kernels of the plan it was captured
 * with: capture again after a change of plan). */
int nnpops_cfconv_set_weights(nnpops_cfconv_t h, const float* w1, const float* b1, const float* w2, const float* b2);

/* ------------------------------------------------------------------------------------------
 * getNeighborPairs (replaces the neighbors::getNeighborPairs CUDA kernels)
 * ------------------------------------------------------------------------------------------ */
/* dtype: 0 = float32, 1 = float64 (positions, box, deltas, distances share it).
 * positions: device [num_atoms][3]; box: device [3][3] or NULL (no periodic wrap);
 * max_num_pairs: -1 = one slot per lower-triangle pair, k -> (row, col<row) as tril_indices;
 *                >0 = compacted list of that many slots.
 * neighbors: device int32 [2][P]; deltas: device [P][3]; distances: device [P]; num_pairs: device int32[1]
 * with P = num_atoms*(num_atoms-1)/2 or max_num_pairs.  All four are fully written:
 * unused slots hold -1 / NaN / NaN (getNeighborPairsCUDA.cu:137-139); num_pairs receives the number
 * of pairs within the cutoff, which may exceed P in compacted mode (surplus pairs are dropped).
 * In compacted mode the list is emitted in ascending pair order (deterministic, unlike the reference).
 * workspace: device scratch of at least nnpops_neighbor_pairs_workspace_bytes(num_atoms) bytes. */
int64_t nnpops_neighbor_pairs_workspace_bytes(int num_atoms);
int nnpops_neighbor_pairs_forward(int dtype, int num_atoms, const void* positions, const void* box, double cutoff,
                                  int64_t max_num_pairs, int32_t* neighbors, void* deltas, void* distances,
                                  int32_t* num_pairs, void* workspace, void* stream);
/* The cell grid that the last nnpops_neighbor_pairs_forward() with this workspace and this num_atoms left in it (compacted lists of
 * 8 192 atoms and more; anything else builds no grid and the words are whatever the workspace held), as nnpops_ani_read_grid:
 * out = {nx, ny, nz, ncells, m, ok, bin_overflow, periodic}.  Waits for `stream`, runs no kernel, not capturable; diagnostics only. */
int nnpops_neighbor_pairs_read_grid(const void* workspace, int num_atoms, void* stream, int32_t* out);
/* grad_positions: device [num_atoms][3], fully overwritten
 * (getNeighborPairsCUDA.cu:80-101: +g on neighbors[0], -g on neighbors[1], g = grad_deltas + deltas/distance*grad_distances). */
int nnpops_neighbor_pairs_backward(int dtype, int num_atoms, int64_t num_slots, const int32_t* neighbors,
                                   const void* deltas, const void* distances, const void* grad_deltas,
                                   const void* grad_distances, void* grad_positions, void* stream);
/* The same with caller-provided scratch (device, 8-byte aligned, nnpops_neighbor_pairs_backward_workspace_bytes(num_atoms) bytes;
 * the entry point above takes it from the stream-ordered allocator).  Where the reference adds six floating-point atomics per pair
 * (getNeighborPairsCUDA.cu:96-100), the contributions are added as fixed-point numbers (two 64-bit words per component) on one
 * scale for the call: the result does not depend on the order of the additions -- bitwise reproducible -- and is within 2^-80 of
 * the largest contribution per term of the exact sum.  A NaN / infinite contribution makes the gradients of ITS two atoms NaN
 * (the atoms the reference's atomicAdds poison) and leaves the others what they are without it. */
int64_t nnpops_neighbor_pairs_backward_workspace_bytes(int num_atoms);
int nnpops_neighbor_pairs_backward_ws(int dtype, int num_atoms, int64_t num_slots, const int32_t* neighbors,
                                      const void* deltas, const void* distances, const void* grad_deltas,
                                      const void* grad_distances, void* grad_positions, void* workspace, void* stream);

/* Backward WITHOUT atomics for a list the forward op emitted (round 6; replaces the atomicAdd scatter of getNeighborPairsCUDA.cu:80-101
 * by an owner-computes gather).  Such a list is grouped by neighbors[0] (rows ascending, see above); nnpops_neighbor_pairs_build_index
 * adds the TRANSPOSED view -- the slots sorted by neighbors[1], ascending slot inside an atom's group -- plus the first / last slot of
 * every atom's group on either side.  The list must be COMPACTED, as the forward op emits it when max_num_pairs > 0: the used slots
 * first, grouped by neighbors[0], and -1 only behind them (a tile whose first slot is -1 is skipped whole).  A max_num_pairs == -1
 * list, whose -1 slots are interleaved with the pairs, must go through nnpops_neighbor_pairs_backward_ws.  A slot whose neighbors[1]
 * lies outside [0, num_atoms) is dropped from the transposed view like an unused slot (it stays in its row's run of slots).
 *   index: device int32 [nnpops_neighbor_pairs_index_ints(num_atoms, num_slots)], 8-byte aligned; a function of `neighbors` alone, so
 *          the torch op builds it once in forward() when the positions require a gradient and saves it with the list;
 *   workspace: device scratch, 256-byte aligned, nnpops_neighbor_pairs_index_workspace_bytes(...) bytes (free after the call).
 * nnpops_neighbor_pairs_backward_indexed then computes the same grad_positions as nnpops_neighbor_pairs_backward_ws: one pass forms
 * g for every slot, one pass adds them up per atom (float64 accumulation, fixed order: bitwise reproducible; a NaN / infinite g
 * reaches exactly the two atoms of its pair, as the reference's atomics do); workspace: 32-byte aligned,
 * nnpops_neighbor_pairs_backward_indexed_workspace_bytes(dtype, num_slots) bytes.  A list that is NOT grouped by neighbors[0] (edited,
 * shuffled, of unknown origin) must go through nnpops_neighbor_pairs_backward_ws, which assumes nothing.  Additive. */
#define NNPOPS_PAIRS_INDEX_MAX_ATOMS 262144      /* nnpops_neighbor_pairs_build_index: 512 buckets of up to 512 atoms; beyond, NNPOPS_ERR_UNSUPPORTED */
int64_t nnpops_neighbor_pairs_index_ints(int num_atoms, int64_t num_slots);
int64_t nnpops_neighbor_pairs_index_workspace_bytes(int num_atoms, int64_t num_slots);
int nnpops_neighbor_pairs_build_index(int num_atoms, int64_t num_slots, const int32_t* neighbors, int32_t* index, void* workspace,
                                      void* stream);
int64_t nnpops_neighbor_pairs_backward_indexed_workspace_bytes(int dtype, int64_t num_slots);
int nnpops_neighbor_pairs_backward_indexed(int dtype, int num_atoms, int64_t num_slots, const int32_t* neighbors, const void* deltas,
                                           const void* distances, const void* grad_deltas, const void* grad_distances,
                                           const int32_t* index, void* grad_positions, void* workspace, void* stream);

/* Box gradient and second derivatives of the backward pass above (additive).  For a used slot k (i = neighbors[0][k],
 * j = neighbors[1][k], both in [0, num_atoms); any other slot is unused and contributes nothing), delta_k = x_i - x_j - sum_a n_ka B[a,:]
 * with n_k the integer minimum-image shift, recovered from positions, box and delta_k (the wrap's rounds have zero derivative);
 * G_k = grad_deltas[k] + deltas[k] / distances[k] * grad_distances[k] as in the backward pass.  box, gg_box, grad_box: [3][3], rows =
 * box vectors (lower triangular, as the forward op takes them), same dtype as positions.  Neither entry needs the transposed index:
 * both work on any list, compacted or max_num_pairs == -1, in any order.  No atomics, no host synchronisation (graph-capturable);
 * bitwise reproducible.  A used slot with distance 0 divides by zero, as the backward pass does.
 *
 * nnpops_neighbor_pairs_box_backward: grad_box[a][:] = - sum_k n_ka G_k (all nine entries, as the reference's CPU composition
 *   differentiates whole rows), added up in float64 per block in a fixed order and then over the blocks in a fixed order.
 *   workspace: device, 8-byte aligned, nnpops_neighbor_pairs_box_backward_workspace_bytes(num_slots) bytes.
 * nnpops_neighbor_pairs_double_backward: vector-Jacobian product of the backward pass, (grad_deltas, grad_distances, deltas, distances)
 *   -> (grad_positions, grad_box), with the incoming gg_positions [num_atoms][3] and gg_box [3][3] (either may be NULL: zero).  Per slot,
 *   w_k = gg_positions[i] - gg_positions[j] - sum_a n_ka gg_box[a][:] and u_k = deltas[k] / distances[k]:
 *     d_grad_deltas[k] = w_k,  d_grad_distances[k] = u_k . w_k,  d_deltas[k] = grad_distances[k] / distances[k] w_k,
 *     d_distances[k] = - grad_distances[k] (deltas[k] . w_k) / distances[k]^2
 *   ([num_slots][3], [num_slots], [num_slots][3], [num_slots]: every slot written, zeros for unused ones).  positions and box are read
 *   only when gg_box is given (then both are required); grad_deltas does not enter. */
int64_t nnpops_neighbor_pairs_box_backward_workspace_bytes(int64_t num_slots);
int nnpops_neighbor_pairs_box_backward(int dtype, int num_atoms, int64_t num_slots, const int32_t* neighbors, const void* positions,
                                       const void* box, const void* deltas, const void* distances, const void* grad_deltas,
                                       const void* grad_distances, void* grad_box, void* workspace, void* stream);
int nnpops_neighbor_pairs_double_backward(int dtype, int num_atoms, int64_t num_slots, const int32_t* neighbors, const void* positions,
                                          const void* box, const void* deltas, const void* distances, const void* grad_distances,
                                          const void* gg_positions, const void* gg_box, void* d_grad_deltas, void* d_grad_distances,
                                          void* d_deltas, void* d_distances, void* stream);

/* ------------------------------------------------------------------------------------------
 * PME, direct-space part (replaces computeDirect: src/pytorch/pme/pmeCUDA.cu:30-100, pmeCPU.cpp:75-163) -- the immediate
 * consumer of the pair list above (src/pytorch/pme/pme.py:163-165).  The reciprocal-space part follows below
 * (nnpops_pme_reciprocal_*).
 * ------------------------------------------------------------------------------------------ */
/* positions: device [num_atoms][3]; charges: device [num_atoms]; neighbors int32 [2][num_pairs], deltas [num_pairs][3],
 * distances [num_pairs]: the outputs of nnpops_neighbor_pairs_forward (float32), slots holding -1 are skipped;
 * exclusions: device int32 [num_atoms][max_exclusions], every row sorted in DESCENDING order and padded with -1, symmetric
 * (pme.py:66-73,93); may be NULL when max_exclusions == 0.  alpha: Ewald splitting parameter; coulomb: 1/(4 pi eps0) in the
 * caller's units.  energy: device float[1]; position_deriv: device [num_atoms][3] = dE/dpositions; charge_deriv: device
 * [num_atoms] = dE/dcharges; all three fully overwritten.  workspace: device scratch of at least
 * nnpops_pme_direct_workspace_bytes(...) bytes -- about num_atoms x min(4 x num_pairs / num_atoms + 32, 2048) x 16 bytes (a row of
 * incoming contributions per atom; num_pairs is the capacity of the list, so a heavily padded list costs workspace up to that
 * clamp: 32 KiB per atom).  The table of exclusions must be SYMMETRIC: every atom takes the terms of its excluded pairs from its own
 * row (the Python wrapper checks it once).  Graph-capturable.
 * Reproducibility: the energy is bitwise reproducible for every list.  The derivatives of an atom are bitwise reproducible as long as
 * the atom receives no more entries than its row holds: cap = min(4 x ceil(num_pairs / num_atoms) + 32, 2048), one entry per
 * included pair the atom is second in and one per run of consecutive slots (within 64 aligned slots) it is first in.  Entries beyond
 * cap -- a dense cluster among dilute atoms, a hub atom, any all-pairs list of more than 2 049 atoms -- are added with float atomics
 * in the order they arrive: such an atom's derivatives are correct to float32 rounding but NOT bitwise reproducible from call to call.
 * nnpops_pme_direct_indexed below has no such limit. */
int64_t nnpops_pme_direct_workspace_bytes(int64_t num_pairs, int num_atoms, int max_exclusions);
int nnpops_pme_direct(int num_atoms, int64_t num_pairs, int max_exclusions, const float* positions, const float* charges,
                      const int32_t* neighbors, const float* deltas, const float* distances, const int32_t* exclusions,
                      float alpha, float coulomb, float* energy, float* position_deriv, float* charge_deriv, void* workspace,
                      void* stream);
/* The same sums over the pair list's transposed index (round 6: nnpops_neighbor_pairs_build_index above) for a list the forward op of
 * getNeighborPairs emitted: one streaming pass over the slots + an owner-computes gather, no atomics, no rows of incoming entries,
 * float64 accumulation in a fixed order (bitwise reproducible).  `index` must have been built from exactly this `neighbors`; workspace:
 * nnpops_pme_direct_indexed_workspace_bytes(num_pairs, num_atoms) bytes (32 bytes per slot).  Everything else as nnpops_pme_direct,
 * which remains the entry point for lists of unknown origin.  Additive. */
int64_t nnpops_pme_direct_indexed_workspace_bytes(int64_t num_pairs, int num_atoms);
int nnpops_pme_direct_indexed(int num_atoms, int64_t num_pairs, int max_exclusions, const float* positions, const float* charges,
                              const int32_t* neighbors, const float* deltas, const float* distances, const int32_t* exclusions,
                              const int32_t* index, float alpha, float coulomb, float* energy, float* position_deriv,
                              float* charge_deriv, void* workspace, void* stream);
/* Box gradient of the direct-space energy above (additive): grad_box [3][3] (device float32, rows = box vectors, all nine entries)
 * = dE/dB = - sum_k n_k (x) G_k over the included pairs (both atoms in [0, num_atoms), not excluded), G_k = dE/ddelta_k =
 * -dedr_k deltas[k] with the direct kernels' dedr, n_k the slot's integer minimum-image shift recovered from positions, box_vectors
 * and deltas[k] (box_vectors: device float32 [3][3], reduced triclinic, the box the list was built with).  Excluded pairs are taken
 * un-wrapped and add nothing.  Any list order, -1 slots anywhere; it only reads the list, so it serves lists with and without a
 * transposed index.  Float64 sums per block in a fixed order, then over the blocks in a fixed order: bitwise reproducible, no
 * atomics, no host synchronisation (graph-capturable).  workspace: device, 8-byte aligned,
 * nnpops_pme_direct_box_workspace_bytes(num_pairs) bytes. */
int64_t nnpops_pme_direct_box_workspace_bytes(int64_t num_pairs);
int nnpops_pme_direct_box(int num_atoms, int64_t num_pairs, int max_exclusions, const float* positions, const float* charges,
                          const int32_t* neighbors, const float* deltas, const float* distances, const int32_t* exclusions,
                          const float* box_vectors, float alpha, float coulomb, float* grad_box, void* workspace, void* stream);
/* Double backward of the direct-space energy with respect to positions and charges (additive; force matching).  With P = dE/dpositions
 * and C = dE/dcharges of the entries above and the cotangents v (device float32 [num_atoms][3]) and w (device [num_atoms]):
 *     grad_positions [num_atoms][3] = d/dpositions,  grad_charges [num_atoms] = d/dcharges  of  L = sum_i v_i . P_i + sum_i w_i C_i
 * (both fully overwritten; the caller scales them by the energy's grad_output).  deltas / distances enter as data: the image shifts
 * are held fixed, as in the first-order entries.  Excluded pairs un-wrapped, every atom from its own row (symmetric table).
 * Owner computes over the list's transposed index, no atomics of any kind, float64 sums in a fixed order: bitwise reproducible; no
 * host synchronisation (graph-capturable).
 *   index: nnpops_neighbor_pairs_build_index of `neighbors` -- required;
 *   first_index: NULL for a list grouped by neighbors[0] (what the forward op of getNeighborPairs emits: `index`'s row segments are
 *     used); for any other list the index built from the list with its two rows swapped ([neighbors[1]; neighbors[0]]), whose column
 *     segments then serve the first side.  build_index drops slots whose column is outside [0, num_atoms) and skips a tile that
 *     STARTS with a negative column, so for a list with -1 slots among the pairs build both indices from a copy in which the
 *     negative entries are replaced by num_atoms (the torch op does exactly that).
 *   workspace: nnpops_pme_direct_double_backward_workspace_bytes(num_pairs, num_atoms) bytes (32 bytes per slot). */
int64_t nnpops_pme_direct_double_backward_workspace_bytes(int64_t num_pairs, int num_atoms);
int nnpops_pme_direct_double_backward(int num_atoms, int64_t num_pairs, int max_exclusions, const float* positions, const float* charges,
                                      const int32_t* neighbors, const float* deltas, const float* distances, const int32_t* exclusions,
                                      const int32_t* index, const int32_t* first_index, const float* v, const float* w, float alpha,
                                      float coulomb, float* grad_positions, float* grad_charges, void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------
 * PME, reciprocal-space part (replaces computeReciprocal: src/pytorch/pme/pmeCUDA.cu:102-430, pmeCPU.cpp:174-364).  Three passes
 * around two FFTs that are the CALLER's (torch.fft / hipFFT; this library links no FFT):
 *   1. nnpops_pme_reciprocal_spread: positions, charges -> real grid float32 [gridx][gridy][gridz] (fully overwritten):
 *      sum over atoms of q sqrt(coulomb) thx thy thz at (base + i) mod grid, B-splines of `order` (4 or 5);
 *   2. the caller: complex grid = rfftn(real grid) with the DEFAULT norm (unscaled forward transform), complex64
 *      [gridx][gridy][gridz / 2 + 1], contiguous;
 *   3. nnpops_pme_reciprocal_convolve: multiplies the complex grid IN PLACE by exp(-pi^2 m^2 / alpha^2) / (pi V m^2 bx by bz)
 *      (0 at m = 0; bx, by, bz the B-spline moduli, device float32 [gridx], [gridy], [gridz]) and writes energy (device float[1])
 *      = 0.5 sum_k w |S(k)|^2 eterm, w = 2 for 0 < kz <= (gridz - 1) / 2, else 1.  The self energy is NOT included.
 *   4. the caller: real grid = irfftn(scaled complex grid, s = (gridx, gridy, gridz), norm = "forward") (unscaled inverse);
 *   5. nnpops_pme_reciprocal_interpolate: dE/dpositions [num_atoms][3] and dE/dcharges [num_atoms] (fully overwritten) from
 *      the weights spread stored in the workspace.
 * box_vectors: device float32 [3][3], reduced triclinic (a = (a0, 0, 0), b = (b0, b1, 0), c = (c0, c1, c2)), read on the device by
 * every pass (never copied to the host).  workspace: device scratch of nnpops_pme_reciprocal_workspace_bytes(...) bytes, the SAME
 * buffer with the same sizes for all three calls of one evaluation (spread stores the splines in it for interpolate).  No float
 * atomics: the grid, the energy and the derivatives are bitwise reproducible.  Orders other than 4 and 5: NNPOPS_ERR_INVALID_ARGUMENT.
 * Graph-capturable.  Additive. */
int64_t nnpops_pme_reciprocal_workspace_bytes(int num_atoms, int gridx, int gridy, int gridz, int order);
int nnpops_pme_reciprocal_spread(int num_atoms, int gridx, int gridy, int gridz, int order, const float* positions, const float* charges,
                                 const float* box_vectors, float coulomb, float* real_grid, void* workspace, void* stream);
int nnpops_pme_reciprocal_convolve(int num_atoms, int gridx, int gridy, int gridz, int order, const float* box_vectors, float alpha,
                                   const float* xmoduli, const float* ymoduli, const float* zmoduli, void* recip_grid, float* energy,
                                   void* workspace, void* stream);
int nnpops_pme_reciprocal_interpolate(int num_atoms, int gridx, int gridy, int gridz, int order, const float* charges,
                                      const float* box_vectors, float coulomb, const float* real_grid, float* position_deriv,
                                      float* charge_deriv, void* workspace, void* stream);
/* Box gradient of the reciprocal-space energy (additive).  With E = 0.5 sum_k w E'_k (E'_k = eterm |S(k)|^2, the sum of step 3),
 * b = pi^2 / alpha^2, m_k = B^-1 k and g_j = dE/dx_j (step 5):
 *     grad_box = dE/dB = - B^-T (Pi + X),  Pi = 0.5 sum_{k != 0} w E'_k [I - 2 (b + 1/|m_k|^2) m_k m_k^T],  X = sum_j x_j (x) g_j
 * (positions held fixed as passed, not wrapped; all nine entries).  Two entries take the place of / follow the steps above:
 *   3'. nnpops_pme_reciprocal_convolve_box: step 3 -- the same scaled grid and energy, bit for bit -- that also leaves the per-workgroup
 *       float64 sums of Pi in box_workspace;
 *   6.  nnpops_pme_reciprocal_box_gradient: after step 5, X from positions and position_deriv (the unscaled dE/dpositions of step 5),
 *       then grad_box (device float32 [3][3]) = - B^-T (Pi + X), B^-1 the general 3 x 3 inverse in float64.
 * box_workspace: device scratch of nnpops_pme_reciprocal_box_workspace_bytes(...) bytes, the same buffer for 3' and 6 (the step-3
 * workspace keeps its size).  Fixed-order float64 sums, no atomics: bitwise reproducible.  Graph-capturable. */
int64_t nnpops_pme_reciprocal_box_workspace_bytes(int num_atoms, int gridx, int gridy, int gridz, int order);
int nnpops_pme_reciprocal_convolve_box(int num_atoms, int gridx, int gridy, int gridz, int order, const float* box_vectors, float alpha,
                                       const float* xmoduli, const float* ymoduli, const float* zmoduli, void* recip_grid, float* energy,
                                       void* workspace, void* box_workspace, void* stream);
int nnpops_pme_reciprocal_box_gradient(int num_atoms, int gridx, int gridy, int gridz, int order, const float* positions,
                                       const float* box_vectors, const float* position_deriv, float* grad_box, void* box_workspace,
                                       void* stream);
/* Double backward of the reciprocal-space energy with respect to positions and charges (additive; force matching).  W_i(m): atom i's
 * separable B-spline weight at grid point m; phi: the real grid of step 4 (the potential).  With the cotangents v (device float32
 * [num_atoms][3], of dE/dpositions) and w (device [num_atoms], of dE/dcharges), L = sum_i v_i . dE/dx_i + sum_i w_i dE/dq_i:
 *   7. nnpops_pme_reciprocal_spread_directional: real grid (fully overwritten) Q' = sqrt(coulomb) sum_i [w_i W_i + q_i (v_i . grad) W_i],
 *      over the bricks and sorted atoms step 1 left in `workspace` (same positions: no second sort); also fills second_workspace;
 *   8. the caller: rfftn(Q') -> nnpops_pme_reciprocal_convolve (its energy output is not needed) -> irfftn(norm = "forward") = phi';
 *   9. nnpops_pme_reciprocal_interpolate_second: from phi (potential_grid) and phi' (directional_grid)
 *        grad_charges[j]   = sqrt(coulomb) [W_j . phi' + ((v_j . grad) W_j) . phi]
 *        grad_positions[j] = sqrt(coulomb) [q_j grad W_j . phi' + q_j grad((v_j . grad) W_j) . phi + w_j grad W_j . phi]
 *      (both fully overwritten; the caller scales them by the energy's grad_output).
 * workspace: the buffer of steps 1-5 of the SAME evaluation, unchanged since (steps 7-9 only read its splines and bricks; step 8
 * overwrites its energy partials).  second_workspace: nnpops_pme_reciprocal_second_workspace_bytes(...) bytes, the same buffer for 7 and 9
 * (the spline weights and their first and second differences in double, and the fractional directions).  positions, charges, box_vectors: as passed to step 1.  Orders 4 and 5.
 * No atomics: bitwise reproducible.  No host synchronisation (graph-capturable). */
int64_t nnpops_pme_reciprocal_second_workspace_bytes(int num_atoms, int gridx, int gridy, int gridz, int order);
int nnpops_pme_reciprocal_spread_directional(int num_atoms, int gridx, int gridy, int gridz, int order, const float* positions,
                                             const float* charges, const float* box_vectors, float coulomb, const float* v, const float* w,
                                             float* real_grid, void* workspace, void* second_workspace, void* stream);
int nnpops_pme_reciprocal_interpolate_second(int num_atoms, int gridx, int gridy, int gridz, int order, const float* charges,
                                             const float* box_vectors, float coulomb, const float* w, const float* potential_grid,
                                             const float* directional_grid, float* grad_positions, float* grad_charges, void* workspace,
                                             void* second_workspace, void* stream);

/* ---- dense layers of the ANI atomic networks (reference src/pytorch/BatchedNN.cpp:30-50, BatchedNN.py:37-122) ----
 * C[M x N] = A[M x K] B with fp32 in and out; the products run on the half-precision matrix instruction with every
 * operand carried as two fp16 planes (22 significant bits) and fp32 accumulation.  B arrives pre-split:
 * nnpops_split_planes writes the planes [rows][ldp] (ldp a multiple of 32, zero padded) of W [rows][cols] -- or of its
 * transpose: rows/cols then describe the OUTPUT, W is [cols][rows].  For y = x W^T with a torch Linear weight
 * W [out][in], B = planes(W) with rows = N = out, cols = K = in.  All pointers are device pointers. */
int nnpops_split_planes(void* stream, int rows, int cols, const float* w, long ldw, int transpose, void* hi, void* lo, long ldp);
/* batch: independent problems `stride*` elements apart (0 = shared operand).
 * epilogue 0: none; 1: C = CELU(C + bias[N], alpha); 2: C *= CELU'(Y) with Y [M][ldy] a saved CELU OUTPUT.
 * prologue 0: A as given; 1: A[m][k] = pv[k] * CELU'(PY[m][k]) (A itself is not read).
 * a_scale: A is multiplied by it before the split (and C divided by it): keep |A| * a_scale below 6e4.
 * a_rows / c_rows (optional, batch == 1): row m of A is read from row a_rows[m], row m of C is written to row c_rows[m]
 * -- the atoms of a species need not be gathered into a contiguous block first, nor their gradients scattered back. */
/* out[m] = A[m][0..K) . w + bias (the networks' last layer: one output per member, summed over the members); with
 * out_rows the result of row m goes to out[out_rows[m]]. */
int nnpops_rows_dot(void* stream, int M, int K, const float* A, long lda, const float* w, float bias, float* out, const int* out_rows);
int nnpops_gemm_split(void* stream, int M, int N, int K, int batch, const float* A, long lda, long strideA, const void* Bh,
                      const void* Bl, long ldb, long strideB, float* C, long ldc, long strideC, int epilogue, const float* bias,
                      long strideBias, const float* Y, long ldy, long strideY, int prologue, const float* PY, long ldpy,
                      long stridePY, const float* pv, long stridePv, float alpha, float a_scale, const int* a_rows, const int* c_rows);
/* Which kernel the calling thread's last nnpops_gemm_split launched (host only, no device work): bn = 128 or 64 (columns of a
 * workgroup's tile), k_split = 1 or 2 (2: eight waves, the two halves of every K step added through LDS), fast = 1 when the
 * staging loads took the straight-line 16-byte path (K a multiple of 8, leading dimension and strides multiples of 4 floats,
 * 16-byte aligned bases, NNPOPS_GEMM_FAST not 0).  An error before the thread's first launch; a refused call leaves it unchanged. */
int nnpops_gemm_split_last(int* bn, int* k_split, int* fast);

/* ---- the atomic networks of a whole frame in two launches (replaces the four BatchedLinear + CELU calls and the
 * sum of BatchedNN.py:100-111 inside OptimizedTorchANI.py:49-52, and their autograd backward to the AEV) ----
 * Per atom and ensemble member: Linear(F,H1) CELU Linear(H1,H2) CELU Linear(H2,H3) CELU Linear(H3,1).  The atoms are
 * grouped by species ("kind"): rows[] lists, kind after kind, the row of x (and of dx) that holds each atom's AEV.
 * A workgroup carries 64 atoms of one kind and one member through all four layers with the activations in LDS /
 * registers; with_gradient the same launch runs the backward pass of layers 6, 4 and 2 and leaves dE/dy1 (split fp16
 * planes, workspace d1); nnpops_mlp_input_grad then forms dE/dx = W0^T dE/dy1 and writes the rows of dx.
 * Arithmetic: fp32 in and out; every operand of a product is carried as two fp16 planes (22 significant bits after a
 * scale of 2^-act_scale_log2 -- 1/16 by default --, exact products, fp32 accumulation) -- keep |activation| below 65 504 / scale.
 * Weights arrive packed (nnpops_mlp_pack): W [rows][cols] fp32 -> fragment planes of nnpops_mlp_packed_halves(rows, cols)
 * fp16 values; rows = outputs, cols = inputs of the product the planes are the left operand of.  For a torch Linear
 * weight W_l [out][in] of member m, with widths padded to multiples of 32 (zero rows / columns):
 *   w0  = pack(h1, F,  W_0, permute 0)                     w2 = pack(h2, h1, W_2, permute 1)    w4 = pack(h3, h2, W_4, 1)
 *   w4t = pack(h2, h3, W_4, transpose 1, permute 1)        w2t = pack(h1, h2, W_2, transpose 1, permute 1)
 * members one after the other in each buffer; w0t = pack(F, M*h1, [W_0 of all members stacked: M*h1 x F], transpose 1,
 * permute 1), one buffer for all members.  permute 1 selects the K order in which a matrix-core accumulator hands its
 * rows to the next product (mlp_fused.hip).  Biases b0 [M][h1], b2 [M][h2], b4 [M][h3], last layer w6 [M][h3], b6 [M]. */
#define NNPOPS_MLP_MAX_KINDS 8
typedef struct {
    int num_atoms;                       /* atoms of this kind: the next num_atoms entries of rows[] */
    int h1, h2, h3;                      /* packed layer widths: multiples of 32 in 32..256 */
    const void *w0, *w2, *w4;            /* forward planes (device) */
    const void *w4t, *w2t, *w0t;         /* gradient planes (device; may be NULL when with_gradient == 0) */
    const float *b0, *b2, *b4, *w6, *b6; /* device */
    void* d1;                            /* device workspace, nnpops_mlp_d1_halves(num_atoms, M, h1) fp16 values (gradient only) */
    const void* w0tm;                    /* optional: W_0^T member by member, pack(F, h1, W_0 of member m, transpose 1, permute 1), members one
                                          * after the other -- what the forward launch multiplies dE/dy1 with when the frame has dx_partial */
} nnpops_mlp_kind;
typedef struct {
    int num_kinds, num_features, num_members;
    const float* x; int ldx;             /* device [atoms][ldx], ldx >= num_features, rows 16-byte aligned; num_features % 8 == 0 */
    const int32_t* rows;                 /* device [sum of num_atoms] */
    float* energies;                     /* device [sum of num_atoms][num_members]: output of every (grouped atom, member) network */
    float alpha;                         /* CELU alpha (0.1 in TorchANI) */
    float* dx; int lddx;                 /* nnpops_mlp_input_grad: device [atoms][lddx]; rows listed in rows[] are overwritten */
    const float* upstream;               /* optional device scalar: dx is multiplied by it (dE_total/dE of this sum); NULL = 1 */
    float dx_scale;                      /* host scalar, also multiplied into dx (e.g. 1 / num_members for an ensemble mean); 0 is read as 1 */
    nnpops_mlp_kind kinds[NNPOPS_MLP_MAX_KINDS];
    /* Networks over a SUBSET of the columns of x.  The AEV blocks of species a molecule does not contain are structurally zero
     * (no neighbour of that species, no pair with it): their products need not be formed and their weights not be read.  With
     * x_groups (device, num_features / 16 entries; num_features % 16 == 0) the planes w0 / w0t / w0tm are packed over
     * num_features = 16 * (number of live blocks) columns and feature block f reads columns 16 * x_groups[f] .. + 15 of x (and
     * writes those of dx).  dead_groups lists the other 16-column blocks of dx: nnpops_mlp_input_grad sets them to zero.  The
     * result of the full product whenever the skipped columns of x are zero (up to the order of the fp32 additions: the live
     * columns share K steps differently).  NULL / 0: all columns, as before. */
    const int32_t* x_groups;
    const int32_t* dead_groups; int num_dead_groups;
    /* Optional device workspace [num_members][sum of num_atoms][num_features] floats, for num_features <= 256 and kinds with w0tm:
     * nnpops_mlp_forward(with_gradient) then also forms every member's W_0^T dE/dy1 (d1 never leaves the CU) and
     * nnpops_mlp_input_grad only adds the members up, in a fixed order. */
    float* dx_partial;
    /* Optional, honoured by nnpops_mlp_input_grad when dx_partial is set: the launch that adds the members up also takes the
     * energy mean of nnpops_mlp_energy_mean (mean_out, a device float) or nnpops_mlp_energy_mean_shifted (mean_shift and
     * mean_out_shifted, device doubles) with scale mean_scale -- same numbers, one launch fewer. */
    float mean_scale; float* mean_out; const double* mean_shift; double* mean_out_shifted;
    /* Optional, honoured by nnpops_mlp_forward: its first thread copies *publish_word to publish_to[1] and then stores publish_stamp
     * to publish_to[0] (system scope, release) -- the deferred capacity check of an ANI handle (nnpops_ani_check_begin_with) riding
     * along instead of taking a launch of its own.  All three come from that call; NULL / 0: nothing is published. */
    const int32_t* publish_word; int32_t* publish_to; int32_t publish_stamp;
    /* Operand scale of the fp16 planes: activations (and back-propagated gradients) are split after a scale of 2^-act_scale_log2,
     * so |activation| must stay below 65 504 * 2^act_scale_log2.  0 is read as 4 -- the fixed 1/16 (|activation| < 1e6) of rounds
     * 1-4; 4 .. 12 accepted.  A larger exponent buys range for networks whose weights admit large activations at the price of
     * the smallest activations' last bits (below 6e-5 * 2^act_scale_log2 the high plane is a denormal; the low plane still carries
     * the remainder): callers derive it from a bound on the activations (nnpops_amd/BatchedNN.py: _refresh_planes). */
    int act_scale_log2;
    /* Optional, with mean_out / mean_out_shifted: the rows are num_segments molecules and the mean is taken per molecule
     * (nnpops_mlp_energy_mean_segments below) -- mean_out / mean_out_shifted then hold num_segments values.  segment_offsets
     * [num_segments + 1] and segment_positions [sum of num_atoms] are device arrays; NULL / 0: one mean over everything. */
    const int32_t* segment_offsets; const int32_t* segment_positions; int num_segments;
    /* Optional, honoured by nnpops_mlp_input_grad on both of its paths: one upstream weight per (molecule, member), a device table
     * [num_segments or 1][member_weights_ld] with member_weights_ld >= num_members.  dx is then the gradient of
     * sum_b sum_m member_weights[b][m] * E_m(molecule b) -- member m's share W_0m^T dE_m/dy1 times the weight of the atom's molecule,
     * members in their fixed order -- instead of the gradient of the plain sum over the members (upstream and dx_scale still multiply
     * it).  The atom's molecule is found from segment_offsets / num_segments, which may then be given without the means and without
     * segment_positions; without them every row belongs to molecule 0.  A member whose weight is zero is SKIPPED: its share is not
     * added, whatever it holds.  At most 128 members.  NULL / 0: every weight is 1, as before. */
    const float* member_weights; int member_weights_ld;
} nnpops_mlp_frame;
int64_t nnpops_mlp_packed_halves(int rows, int cols);
int64_t nnpops_mlp_d1_halves(int num_atoms, int num_members, int h1);
int nnpops_mlp_pack(void* stream, int rows, int cols, const float* w, long ldw, int transpose, int permute, void* out);
int nnpops_mlp_forward(void* stream, const nnpops_mlp_frame* frame, int with_gradient);
int nnpops_mlp_input_grad(void* stream, const nnpops_mlp_frame* frame);
/* The packed parameters of a WHOLE ensemble from its eight arrays, on the device: what a trainable module rebuilds after every optimizer
 * step (nnpops_amd/BatchedNN.py: _TrainableFusedNN).  The arrays are contiguous fp32 device arrays in the module's layout, zero padded to
 * the widest kind:
 *   layer0_weights [kinds][M][out0][F]    layer2_weights [kinds][M][out2][in2]    layer4_weights [kinds][M][out4][in4]
 *   layer6_weights [kinds][M][out6][in6]  (row 0 is the output)                   layerL_biases  [kinds][M][outL][1]
 * widths: the packed widths h1, h2, h3 of every kind (host; multiples of 32 in 32..256), each matrix being cut or zero padded to them.
 * nnpops_mlp_pack_networks writes
 *   planes      per kind  w0 (M members) | w2 (M) | w4 (M) | w4t (M) | w2t (M) | w0t  -- the planes nnpops_mlp_pack writes for each of these
 *               matrices (see above), one after the other: nnpops_mlp_networks_plane_halves(nets, 0) fp16 values;
 *   floats      per kind  b0 [M][h1] | b2 [M][h2] | b4 [M][h3] | w6 [M][h3] | b6 [M]: nnpops_mlp_networks_floats(nets) floats;
 *   live_planes (with live_blocks, a device list of num_live_blocks 16-column blocks of the input; else ignored) the same set with the
 *               first layer over the columns of those blocks only (nnpops_mlp_frame: x_groups), and behind w0t, when they are at most 256
 *               columns, w0tm (M): nnpops_mlp_networks_plane_halves(nets, 1) fp16 values;
 *   status      NNPOPS_MLP_PACK_STATUS_BYTES bytes, all a caller needs to decide whether and how the planes can be used, so that ONE small
 *               copy to the host is the only synchronisation of a rebuild:
 *                 int32 [3 * NNPOPS_MLP_MAX_KINDS]  per (kind, layer 0 / 2 / 4): 1 + the last row r for which the weights [:, r, :] or the
 *                                     biases [:, r] of the kind hold a non-zero value and no NaN (over all members and inputs); 0: none
 *                 int32               1 if a value of the weights of any layer or of the biases of layers 0, 2, 4 is not finite
 *                 int32               (padding)
 *                 float64 [9]         the largest row abs-sum of layer 0, 2, 4 weights; the largest column abs-sum of layer 4, layer 2
 *                                     weights; the largest |bias| of layers 0, 2, 4; the largest |layer 6 weight|  (NaNs left out)
 * Two launches whatever the number of kinds, members and matrices; no floating-point atomics; the abs-sums are formed in float64 in a
 * fixed order: repeated calls give the same bits in all four outputs.  planes and live_planes 16-byte aligned, status 8-byte aligned.  A
 * bad descriptor (NULL, widths, num_features % 8, more than NNPOPS_MLP_MAX_KINDS kinds, more than 128 members) returns
 * NNPOPS_ERR_INVALID_ARGUMENT and launches nothing; the size queries then return that code (a negative number). */
#define NNPOPS_MLP_PACK_STATUS_BYTES 176
typedef struct {
    int num_kinds, num_members, num_features;
    int out0, out2, in2, out4, in4, out6, in6;
    const float *layer0_weights, *layer0_biases, *layer2_weights, *layer2_biases;
    const float *layer4_weights, *layer4_biases, *layer6_weights, *layer6_biases;
    int widths[3 * NNPOPS_MLP_MAX_KINDS];
    const int32_t* live_blocks; int num_live_blocks;
} nnpops_mlp_networks;
int64_t nnpops_mlp_networks_plane_halves(const nnpops_mlp_networks* nets, int live);
int64_t nnpops_mlp_networks_floats(const nnpops_mlp_networks* nets);
int nnpops_mlp_pack_networks(void* stream, const nnpops_mlp_networks* nets, void* planes, float* floats, void* live_planes, void* status);
/* The gradient of  sum_b sum_m member_weights[b][m] * E_m(molecule b)  (every weight 1 without the table) with respect to the eight
 * parameter arrays of every kind: fp32 device arrays in torch's Linear layout at the kind's PACKED widths (h1, h2, h3 of
 * nnpops_mlp_kind; rows and columns of the zero padding come out as exact zeros),
 *   dw0 [M][h1][F]  db0 [M][h1]  dw2 [M][h2][h1]  db2 [M][h2]  dw4 [M][h3][h2]  db4 [M][h3]  dw6 [M][h3]  db6 [M]
 * with F = num_features: with x_groups the live width, column f of dw0 belonging to column 16 x_groups[f / 16] + f % 16 of x (the
 * gradient of the dead columns is zero, x being zero there).  The call is SELF-CONTAINED: it runs the networks over the frame's x
 * again (it needs a frame that could take nnpops_mlp_forward(frame, 1): transposed planes, d1 or dx_partial) and reads or writes
 * none of energies, d1, dx_partial and dx, so it may come before, between or after nnpops_mlp_forward and nnpops_mlp_input_grad.
 * It honours member_weights, member_weights_ld, segment_offsets, num_segments, x_groups and act_scale_log2 of the frame.
 * Deterministic: no atomics; every value is one wave's sum over the atoms of the kind in their order in rows[] -- fp32 inside the
 * matrix instructions for the four matrices, float64 for the bias sums -- so two calls give the same bits.  A member whose weight is
 * zero for every molecule is skipped and its gradients are zeros; kinds without atoms and frames without atoms give zeros.
 * workspace: nnpops_mlp_weight_grad_workspace_bytes(frame) bytes of device memory, 16-byte aligned -- per-atom data only, (2 (h1 +
 * h2 + h3) + 1) floats per atom (rounded up to 64 per kind) and member; no partial sums. */
typedef struct {
    float *dw0, *db0, *dw2, *db2, *dw4, *db4, *dw6, *db6;
} nnpops_mlp_weight_grad_kind;
typedef struct {
    void* workspace; int64_t workspace_bytes;
    nnpops_mlp_weight_grad_kind kinds[NNPOPS_MLP_MAX_KINDS];
} nnpops_mlp_weight_grad_out;
int64_t nnpops_mlp_weight_grad_workspace_bytes(const nnpops_mlp_frame* frame);
int nnpops_mlp_weight_grad(void* stream, const nnpops_mlp_frame* frame, const nnpops_mlp_weight_grad_out* out);
/* The gradient, in the same eight parameter arrays (shapes and padding as above), of a DIRECTIONAL DERIVATIVE of the networks:
 *   M = sum_b sum_m member_weights[b][m] sum_{atoms a of molecule b} < t_a, dE_m(a)/dx_a >
 * -- what a loss on forces asks for: t is the cotangent of the input gradient (through the AEV: its tangent J.v).  db6 is exactly zero.
 * t: device [atoms][ldt] floats, rows and columns as x of the frame (with x_groups the columns outside the live blocks are not read
 * and get a zero gradient); 16-byte aligned rows, ldt >= num_features, any magnitude (each row is normalised by a power of two inside).
 * tangent_energies (optional): device [sum of num_atoms][num_members] in the grouped order of `energies`: E' = <t_a, dE_m(a)/dx_a>,
 * UNWEIGHTED -- its sum over a molecule's atoms is dM/dmember_weights[b][m].
 * The contract is nnpops_mlp_weight_grad's: SELF-CONTAINED (it runs the networks over the frame's x again and reads or writes none of
 * energies, d1, dx_partial, dx); it honours member_weights(_ld), segment_offsets, num_segments, x_groups and act_scale_log2;
 * deterministic (no atomics, no partial sums: the same bits every call); a member whose weight is zero for every molecule is
 * skipped and gives zeros; kinds or frames without atoms give zeros; a bad descriptor returns NNPOPS_ERR_INVALID_ARGUMENT and launches
 * nothing.  workspace: nnpops_mlp_weight_grad_tangent_workspace_bytes(frame) bytes, 16-byte aligned: (4 h1 + 4 h2 + 3 h3) floats per
 * atom (rounded up to 32 per kind) and member. */
typedef struct {
    const float* t; int ldt;
    void* workspace; int64_t workspace_bytes;
    float* tangent_energies;
    nnpops_mlp_weight_grad_kind kinds[NNPOPS_MLP_MAX_KINDS];
} nnpops_mlp_weight_grad_tangent_out;
int64_t nnpops_mlp_weight_grad_tangent_workspace_bytes(const nnpops_mlp_frame* frame);
int nnpops_mlp_weight_grad_tangent(void* stream, const nnpops_mlp_frame* frame, const nnpops_mlp_weight_grad_tangent_out* out);
/* out[0] = scale * sum(energies[0 .. count)) in double precision and a fixed order: the sum over atoms and the mean over
 * members of BatchedNN.py:109 (scale = 1 / num_members) in one small launch.  Device pointers. */
int nnpops_mlp_energy_mean(void* stream, const float* energies, int64_t count, float scale, float* out);
/* The same sum, promoted to double and shifted by the molecule's self energy: out[0] = (double)(float)(scale * sum) + shift[0] --
 * the `energies + self_energies` of the reference's EnergyShifter (pytorch/EnergyShifter.py:52) without a launch of its own.
 * `shift` and `out` are device doubles. */
int nnpops_mlp_energy_mean_shifted(void* stream, const float* energies, int64_t count, float scale, const double* shift, double* out);
/* out[i] = in[i] * (float)factor[0] for i < count; `factor` is a DEVICE scalar, a double when factor_is_double != 0 and a float
 * otherwise.  The backward of the one-node OptimizedTorchANI step (pytorch/OptimizedTorchANI.py:49-52): forces kept by the forward
 * pass times the gradient autograd hands in, in one launch. */
int nnpops_scale_by_scalar(void* stream, const float* in, int64_t count, const void* factor, int factor_is_double, float* out);
/* The energy mean of nnpops_mlp_energy_mean for a BATCH of molecules: out[b] = scale * sum over the atoms a of molecule b and the
 * members m of energies[positions[a]][m].  `energies` is [num_atoms][num_members] in the grouped order nnpops_mlp_forward writes;
 * molecule b is the rows molecule_offsets[b] .. molecule_offsets[b + 1] - 1 (the convention of nnpops_ani_set_molecules; the
 * offsets start at 0 and end at num_atoms) and positions[row] is the place of that row in the grouped order (the inverse of the
 * frame's rows[]).  All device pointers; 1 <= num_molecules.  One wave per molecule: lane l adds the atoms l, l + 64, ... of the
 * molecule, each atom's members in order, in double precision, and the 64 lane sums meet in a fixed butterfly -- the value of a
 * molecule depends on its own atoms only: not on the number of molecules, on its place among them or on the atoms of other
 * molecules, and no atomic is involved.  Molecules of any size (also empty ones: 0). */
int nnpops_mlp_energy_mean_segments(void* stream, const float* energies, int num_atoms, int num_members, const int32_t* molecule_offsets,
                                    int num_molecules, const int32_t* positions, float scale, float* out);
/* ... promoted and shifted like nnpops_mlp_energy_mean_shifted: out[b] = (double)(float)mean_b + shift[0], device doubles. */
int nnpops_mlp_energy_mean_segments_shifted(void* stream, const float* energies, int num_atoms, int num_members,
                                            const int32_t* molecule_offsets, int num_molecules, const int32_t* positions, float scale,
                                            const double* shift, double* out);
/* The energy of every ensemble member, molecule by molecule: out[b][m] = sum over the atoms a of molecule b of
 * energies[positions[a]][m], a device [num_molecules][num_members] array (tables as for nnpops_mlp_energy_mean_segments; with
 * molecule_offsets and positions both NULL and num_molecules 1 everything is one molecule in the order it lies in).  One wave per
 * molecule: lane l adds the atoms l, l + 64, ... of the molecule, every member into a float64 accumulator of its own, and the lane sums
 * meet in the fixed butterfly of the means -- a value depends on the molecule's own atoms only, not on the batch or the molecule's
 * place in it. */
int nnpops_mlp_member_sums(void* stream, const float* energies, int num_atoms, int num_members, const int32_t* molecule_offsets,
                           int num_molecules, const int32_t* positions, float* out);
/* ... promoted and shifted: out[b][m] = (double)(float)sum + shift[0], device doubles. */
int nnpops_mlp_member_sums_shifted(void* stream, const float* energies, int num_atoms, int num_members, const int32_t* molecule_offsets,
                                   int num_molecules, const int32_t* positions, const double* shift, double* out);
/* out[row][0..2] = in[row][0..2] * (float)factors[molecule of row] for the num_atoms rows of a batch of molecules (offsets as above);
 * `factors` is a DEVICE array of num_molecules doubles when factor_is_double != 0, floats otherwise.  The backward of the batched
 * one-node step: every molecule's kept forces times its own upstream gradient, in one launch. */
int nnpops_scale_by_segment(void* stream, const float* in, int num_atoms, const int32_t* molecule_offsets, int num_molecules,
                            const void* factors, int factor_is_double, float* out);

#ifdef __cplusplus
}
#endif
#endif /* NNPOPS_HIP_H */
