/* nbe.h -- C ABI of the MI355X-native N-body emulator engine (libnbe.so).
 *
 * The reference (oleg-savchenko/jax_nbody_emulator_with_dj) has no native/FFI boundary: its boundary is
 * the Python API.  Each entry point below names the reference interface it replaces (file:line relative
 * to the reference repository root); the Python shim in jax_nbody_emulator_with_dj_amd/ binds them with
 * ctypes.
 *
 * Conventions: every function returns 0 on success and a non-zero code on failure (1 = error, 2 = NBE_ERANGE, see
 * "Range" below); the message is available from nbe_last_error() (thread local).  No entry point aborts the process.  Tensors are float32, C-contiguous, channel-first
 * ((C, D, H, W)) exactly as the reference passes them.  Data pointers may be host OR device pointers
 * (detected with hipPointerGetAttributes); the caller owns them.  The library owns all device memory it
 * allocates.  One in-flight call per context; several contexts may coexist (one per GPU / stream).
 */
#ifndef NBE_H
#define NBE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nbe_ctx nbe_ctx;

/* progress callback of nbe_process_box: replaces the tqdm bar of src/jax_nbody_emulator/subbox.py:186-193 */
typedef void (*nbe_progress_cb)(int done, int total, void* user);   /* done / total = fraction of the box finished */

/* One convolution layer of the parameter tree {'params': {block: {layer: {...}}}}
 * (leaf shapes: tests/test_style_nbody_emulator_vel_core.py:408-419, style_layers_vel.py:55-75;
 *  premodulated leaves: nbody_emulator.py:256-260).  All pointers are HOST float32. */
typedef struct nbe_layer_desc {
    const char* block;          /* "conv_l00", "down_l0", ...                         */
    const char* layer;          /* "skip", "conv_0", "conv_1"                           */
    int cout, cin, k;           /* weight shape (cout, cin, k, k, k)                    */
    const float* weight;        /* style: raw weight; premodulated: normalised weight   */
    const float* bias;          /* (cout,)                                              */
    const float* style_weight;  /* (cin, 2)  -- style trees only                        */
    const float* style_bias;    /* (cin,)    -- style trees only                        */
    const float* dweight;       /* premodulated velocity trees only, same shape as weight */
} nbe_layer_desc;

enum { NBE_F32 = 0, NBE_F16 = 1, NBE_F64 = 2 };   /* NBE_F64: particle positions only (nbe_paint_particles) */

const char* nbe_last_error(void);
int nbe_version(void);

/* context = one GPU + one stream + weights + workspace.
 * replaces: the implicit JAX device/jit state created by SubboxProcessor.__init__ (subbox.py:106-137) */
int nbe_create(int device_id, nbe_ctx** out);
int nbe_destroy(nbe_ctx* ctx);
/* run on a caller-provided hipStream_t (e.g. torch's current stream) so that the caller's device work before
 * and after a call is ordered with it; NULL = the device's default (null) stream, as everywhere in HIP.
 * A new context runs on its own non-blocking stream (NOT ordered with the null stream); nbe_use_own_stream
 * returns to it.  Both synchronise the stream being left. */
int nbe_set_stream(nbe_ctx* ctx, void* hip_stream);
int nbe_use_own_stream(nbe_ctx* ctx);
int nbe_synchronize(nbe_ctx* ctx);

/* model hyper-parameters: StyleNBodyEmulatorVelCore(style_size=2, in_chan, out_chan, mid_chan, eps)
 * (style_nbody_emulator_vel_core.py:39-43); compute_vel selects the *VelCore / *Core twin
 * (nbody_emulator.py:324-339). */
int nbe_set_arch(nbe_ctx* ctx, int in_chan, int out_chan, int mid_chan, float eps, int compute_vel);

/* Arithmetic of the convolutions (call before loading weights).  The reference selects it through the dtype
 * of x (SubboxConfig.dtype, style_layers_vel.py:103-105); its float32 runs on TF32-class tensor cores.
 *   NBE_PREC_F32    strict float32 MFMA (default)
 *   NBE_PREC_F16X3  float32-equivalent: operands split into two f16 numbers, three f16 MFMAs per product,
 *                   float32 accumulation (22-bit operands; measured whole-network error equal to float32's)
 *   NBE_PREC_F16    plain float16 operands, one f16 MFMA per product, float32 accumulation: the arithmetic of
 *                   the reference's SubboxConfig.dtype = float16 configuration (its fastest rows, README.md:245-250) */
enum { NBE_PREC_F32 = 0, NBE_PREC_F16X3 = 1, NBE_PREC_F16 = 2 };
int nbe_set_precision(nbe_ctx* ctx, int precision);

/* Range of the f16-based modes (NBE_PREC_F16X3, NBE_PREC_F16).  Their operands are f16 numbers (|v| < 65504, full
 * precision above 6.1e-5), while the reference's float32 arithmetic (style_layers_vel.py:103-105) has float32's range.
 * The engine therefore shifts every call into f16's comfortable range: LeakyReLU is positively homogeneous and the
 * convolutions are linear, so f(s x; s b) = s f(x; b) for the network f with input x and biases b, exactly in floating
 * point for s = 2^k.  Per call k is chosen such that max(max|x| * Dz / 6, max|b|) * 2^k lies in [0.5, 1) (NBE_PREC_F16)
 * or in [32, 64) (NBE_PREC_F16X3: the Winograd-z kernel keeps the lo part of its transformed planes unscaled, a normal f16
 * number for every |value| >= 2^-9 of the input's scale there): a reduction over the input, the input scaled in the
 * gather, the biases scaled on the device, 2^-k applied in the head.  Valid inputs: any finite float32 box -- parity
 * with the float64 oracle is tested over 24 decades of input scale (tests/test_gpu_range.py).  What remains out of
 * range is a network whose activations grow beyond 65504 (F16) / 1023 (F16X3) times its largest input / bias (weights far
 * from the unit-norm filters the modulation produces); then an infinity or a NaN reaches the head, which flags it:
 *   - host arrays in/out: the call returns NBE_ERANGE (2) instead of the fields;
 *   - device pointers (asynchronous calls): nbe_check_finite() synchronises and returns NBE_ERANGE if any call since
 *     the last check produced a non-finite value from a finite input.  The Python shim calls it after every call and
 *     recomputes that call on a strict-float32 context (never a silent inf / NaN).
 * Non-finite INPUT values propagate to the outputs as in the reference and are not an error.
 * nbe_set_input_range(ctx, m): use m as max|x| instead of reducing over the input (ranks of a sharded box agree on one
 * value with an all-reduce so that every brick is computed with the same shift); m < 0 returns to the reduction. */
enum { NBE_ERANGE = 2 };
int nbe_check_finite(nbe_ctx* ctx);
int nbe_set_input_range(nbe_ctx* ctx, float absmax);

/* state of the context after the last call / plan: see the enum */
enum { NBE_Q_GAUGE_ACTIVE = 0,     /* 1: the loaded weights run the two-product (gauged) tangent kernels             */
       NBE_Q_SLAB = 1,             /* planes per z-slab of the last plan (0 = whole tensors)                          */
       NBE_Q_PERIODIC_YX = 2,      /* 1: the last plan runs periodic in y and x                                       */
       NBE_Q_PERIODIC_Z = 3,       /* 1: ... and in z                                                                 */
       NBE_Q_RANGE_SHIFT = 4,      /* k of the last call's range shift 2^k                                            */
       NBE_Q_WORKSPACE_BYTES = 5,
       NBE_Q_HOST_PIPE = 6,        /* 1: the last nbe_process_box call ran the pipelined host path (nbe_host_alloc)    */
       NBE_Q_GRAPH_REPLAYS = 7,    /* tiles replayed from a captured hipGraph so far (see below)                       */
       NBE_Q_PLAN_TILES = 8,       /* tiles per box of the last plan                                                    */
       NBE_Q_PLAN_SHORT_GB = 9 };  /* > 0: the last plan is NOT the largest exact merge (max_tile permitting) because its
                                      workspace did not fit: GB of device memory that were missing.  The engine also
                                      writes one line to stderr when that happens (NBE_QUIET=1 silences it): the 512^3
                                      box as one tile needs ~200 GB free beside the box and the fields; with less the
                                      planner takes two, four or eight tiles and runs 1.1 - 1.4 x slower.              */
/* hipGraph replay.  A tile of nbe_process_box / nbe_process_region with device pointers in and out enqueues a few
 * hundred launches (the reference's analogue is the jitted step, subbox.py:137).  The second time the identical tile is
 * requested -- same pointers, geometry, scalars, weights and modulation -- its schedule is captured (on the context's
 * own stream, fenced against the caller's with events), and from the third time on it is ONE hipGraphLaunch.  Results
 * are bit-identical to the eager schedule.  NBE_GRAPH=0 disables it; profiling, progress callbacks and the pipelined
 * host path run eagerly. */
int nbe_query(nbe_ctx* ctx, int what, double* out);

/* replaces model.apply's `params` argument for the Style* cores (README.md:155; subbox.py:224-233) */
int nbe_load_style_weights(nbe_ctx* ctx, const nbe_layer_desc* layers, int nlayers);
/* replaces `params` of the premodulated cores: output of modulate_emulator_parameters[_vel]
 * (nbody_emulator.py:150-187, :221-266) */
int nbe_load_premod_weights(nbe_ctx* ctx, const nbe_layer_desc* layers, int nlayers);

/* Style cores: (Om, Dz) -> style vector s = ((Om-0.3)*5, Dz-1) and the per-layer weight modulation,
 * demodulation and d/dDz (style_nbody_emulator_vel_core.py:126-128, style_layers_vel.py:62-105).
 * Runs the modulate + pack kernels.  No-op for premodulated weights.
 * With velocity (f32 / f16x3) the tangent of style_layers_vel.py:98-105, dy = W.dx + dW.x, is evaluated as
 * W.(dx + alpha x) + beta (W.x) using dW = W (.) (alpha[cin] + beta[cout]) of the style modulation (two contractions
 * per 3x3x3 layer instead of three; same result within rounding).  env NBE_GAUGE=0 at load time keeps the
 * three-product form; a style factor that is exactly zero at (Om, Dz) selects it for that cosmology.
 * f16x3 with velocity: the wide 3x3x3 layers run a Winograd F(2,3) transform along z (conv_h3w_kernel: four plane-wise
 * convolutions per two output planes instead of six, same float32 tolerances).  Its rounding depends on how a launch pairs
 * its planes, so fields of different tilings / slab plans / rank counts agree to float32 rounding, not bit for bit;
 * env NBE_WINO=0 (read per launch) selects the direct kernel, whose rounding is independent of the schedule. */
int nbe_set_cosmology(nbe_ctx* ctx, float Om, float Dz);

/* model.apply(params, x[None], Om, Dz, vel_fac) for ONE batch element
 * (style_nbody_emulator_vel_core.py:105-195 and the three sibling signatures, subbox.py:224-233).
 * x: (in_chan, D, H, W); disp / vel: (out_chan, D-96, H-96, W-96); vel may be NULL when compute_vel=0. */
int nbe_forward(nbe_ctx* ctx, const void* x, int D, int H, int W, float Dz, float vel_fac,
                void* disp, void* vel);

/* SubboxProcessor.process_box (subbox.py:139-219): periodic 48-voxel-halo crops of `box`
 * ((in_chan, size0, size1, size2)), forward, ASSIGNMENT of the un-padded result into disp / vel
 * ((in_chan, size...), out_dtype NBE_F32 or NBE_F16).  Dz, vel_fac: growth_factor / vel_norm scalars
 * (subbox.py:173-178).  pad must be 48 on every side (the model's receptive field, subbox.py:43). */
int nbe_process_box(nbe_ctx* ctx, const void* box, const int64_t size[3], const int ndiv[3], const int pad[6],
                    float Dz, float vel_fac, void* disp, void* vel, int out_dtype,
                    nbe_progress_cb cb, void* user);

/* Pinned host memory from a process-wide pool (hipHostMalloc; freed buffers are kept for reuse up to NBE_PINNED_POOL_GB,
 * default 16).  Host-array calls of nbe_process_box whose OUTPUT arrays come from here are pipelined when the box runs
 * as one periodic tile (the default plan of a 512^3 box on a free MI355X): the input goes up in z-chunks through pinned
 * staging buffers filled by host threads while the first slabs run, and every finished output slab is copied out on a
 * second stream under the kernels of the next -- the reference does gather -> H2D -> compute -> D2H -> paste serially
 * per sub-box (subbox.py:195-215).  Plain (pageable) host arrays work as before, un-overlapped.  The Python shim
 * returns NumPy arrays backed by this pool.  nbe_host_trim releases the pooled buffers. */
void* nbe_host_alloc(size_t bytes);
int nbe_host_free(void* p);
int nbe_host_trim(void);

/* The same loop over a sub-set of the sub-boxes of a REGION of a periodic box (multi-GPU sharding: each
 * rank owns a brick).  Sub-boxes tile [origin, origin+region) with `ndiv`; `order`
 * (nullable) lists the sub-box indices to run, in order; results go to an output array of spatial size
 * out_size at out_origin + anchor.  Outputs are NOT zero-initialised here.  No reference counterpart:
 * the reference loop (subbox.py:195-215) is serial on one device. */
int nbe_process_region(nbe_ctx* ctx, const void* box, const int64_t box_size[3], const int64_t origin[3],
                       const int64_t region[3], const int ndiv[3], const int* order, int norder,
                       float Dz, float vel_fac, void* disp, void* vel, int out_dtype,
                       const int64_t out_size[3], const int64_t out_origin[3]);

/* Brick mode of a sharded box (no reference counterpart: the reference's loop is serial on one device, subbox.py:195-215).
 * The ranks of a node cut the periodic box into slabs along z; a brick is periodic in y and x by itself.  What the network
 * needs from the z neighbours is EXCHANGED at the three places where it is smallest, instead of being recomputed from a
 * 48-plane halo of the raw input:
 *   which 0   4 planes of the raw input per side -- the level-0 encoder's reach beyond the brick ((C, 4, S1, S2) float32);
 *   which 1   6 planes of the down_l0 output per side -- what conv_l1 reads beyond the brick for the level-1 skip connection;
 *   which 2   10 planes of the down_l1 output per side -- what levels 2 and 3 read;
 *   which 3   4 planes of the level-0 skip connection (conv_l01's output) per side -- what the decoder's first block reads
 *             beyond the brick; needed last, it travels while levels 1-3 run.
 * nbe_brick_halo_bytes(ctx, brick_size, which) sizes one such face (device buffers, opaque 16-byte units for 1 - 3).
 *   nbe_brick_encode    haloed_brick = (C, b0 + 8, S1, S2): level-0 encoder on the brick's own planes; writes the first / last
 *                       6 down_l0 planes to send_lo / send_hi and the first / last 4 skip-connection planes to skip_send_*;
 *   nbe_brick_interior  the part of conv_l1 that needs the brick's own planes only -- it runs while the faces travel;
 *   nbe_brick_exchange  with the neighbours' faces (recv_lo = the z-minus neighbour's send_hi, recv_hi = the z-plus
 *                       neighbour's send_lo): the rest of conv_l1, the skip connection, down_l1; writes the first / last
 *                       10 down_l1 planes to send2_lo / send2_hi;
 *   nbe_brick_finish    with the neighbours' second faces and their skip-connection planes: levels 2-3, the decoders, the
 *                       brick's (C, b0, S1, S2) fields.  The skip-connection planes are read last: the stream waits for
 *                       skip_ready_event (recorded by the caller behind their transfer; NULL = they are there) only after
 *                       levels 1-3, so that transfer is hidden under them.
 * The four calls must follow each other on one context (any other call in between invalidates the brick and the next
 * brick call fails); all are asynchronous on the context's stream -- the caller orders the exchanges against it (events).
 * EVERY RANK MUST USE THE SAME RANGE SHIFT: call nbe_set_input_range with the box-wide max |x| first (the shim all-reduces
 * it).  Fields equal the single-device nbe_process_box of the whole box bit for bit, in every arithmetic and for any cut
 * (tests/test_gpu_bricks.py).  conv_h3w_kernel takes a launch only when its plane count is even and pairs the planes from the
 * first one: with b0 % 8 == 0 and origins % 8 == 0, levels 0 - 2 always launch even plane counts from even global planes --
 * the z-slabs inside a brick (nbe_set_slab) included -- and conv_c at level 3, whose b0 / 8 + 6 and b0 / 8 + 4 planes from
 * level-3 plane origin / 8 - 4 are even or odd with the cut, runs on the direct kernels in every call of the engine.
 * b0 must be a multiple of 8, at least 48.  nbe_brick_plan returns the planes per z-slab the brick would run
 * with on the memory that is free now, or 0 when it does not fit (the caller then takes nbe_process_region). */
int64_t nbe_brick_halo_bytes(nbe_ctx* ctx, const int64_t brick_size[3], int which);
int nbe_brick_plan(nbe_ctx* ctx, const int64_t brick_size[3]);
int nbe_brick_encode(nbe_ctx* ctx, const void* haloed_brick, const int64_t brick_size[3], float Dz, float vel_fac,
                     void* send_lo, void* send_hi, void* skip_send_lo, void* skip_send_hi);
int nbe_brick_interior(nbe_ctx* ctx);
int nbe_brick_exchange(nbe_ctx* ctx, const void* recv_lo, const void* recv_hi, void* send2_lo, void* send2_hi);
int nbe_brick_finish(nbe_ctx* ctx, const void* recv2_lo, const void* recv2_hi, const void* skip_recv_lo, const void* skip_recv_hi,
                     void* skip_ready_event /* hipEvent_t or NULL */, float Dz, float vel_fac, void* disp, void* vel, int out_dtype);

/* Internal tiling.  When crop_size = size/ndiv is a multiple of 8 on every axis, all crop origins keep the
 * phase of the network's 2^3 stride lattice, so the per-voxel result does not depend on how the box is cut
 *  and neighbouring sub-boxes can be merged into larger tiles that recompute less halo
 * (17.1 MFLOP/voxel at 128^3 crops, 11.2 at 256^3).  nbe_plan_tiles returns the grid nbe_process_box will
 * with a cubic cap: per axis the largest merge with tile edge <= max_tile; unchanged when crop % 8 != 0.
 * nbe_set_max_tile(ctx, 0) keeps the caller's grid exactly; nbe_set_max_tile(ctx, 256) restricts to 256^3 tiles. */
int nbe_plan_tiles(const int64_t region[3], const int ndiv[3], int max_tile, int out_ndiv[3]);
int nbe_set_max_tile(nbe_ctx* ctx, int max_tile);
/* The grid a context will actually run (weights loaded): among all exact merges with tile edge <= its max_tile
 * (default 512, or env NBE_MAX_TILE) the one with the largest tile whose workspace fits the device memory free at
 * the time of the call, longest along the last axis on ties (512^3 / ndiv 4 on a 288 GB MI355X: four tiles of
 * 256 x 256 x 512).  Falls back to the caller's grid when merging is not exact or no weights are loaded.
 * periodic_box != 0: `region` is a whole periodic box (nbe_process_box); tiles that span it in y and x then run in
 * periodic-yx mode (no halo recompute in y and x at the two full-resolution levels, a smaller workspace). */
int nbe_plan_tiles_ctx(nbe_ctx* ctx, const int64_t region[3], const int ndiv[3], int periodic_box, int out_ndiv[3]);
/* Schedule of the two full-resolution levels of the U-Net inside a tile: whole tensors, or slabs of `slab` output
 * planes along z (even; the slab-sized tensors let a tile be as deep as the box: 512^3 runs as ONE tile).  Results are
 * identical.  -1 (default, or env NBE_SLAB): chosen with the tiling by the memory that is free; 0: never; S: always
 * (a brick plan that nbe_brick_plan / nbe_brick_encode cached under the previous setting is dropped). */
int nbe_set_slab(nbe_ctx* ctx, int slab);
/* Periodic-yx mode (default on, env NBE_PERIODIC=0 off): a tile of nbe_process_box that spans the periodic box in y
 * and x supplies the 48 voxels of y/x context of the two full-resolution levels layer by layer (1-voxel wrap-around
 * halos) instead of padding the input by 48 and shrinking.  Same arithmetic per voxel, ~10 % fewer FLOPs at 512^3. */
int nbe_set_periodic(nbe_ctx* ctx, int on);

/* growth_factor / vel_norm (cosmology.py:34-40, :130-141) in double precision on the host. */
double nbe_growth_factor(double z, double Om);
double nbe_vel_norm(double z, double Om);

/* ---- Density (no context: painting has no weights) -----------------------------------------------
 * The fork's pipeline turns the emulated displacement into a density field right after process_box (scripts/core.py:447-458).
 * All pointers are DEVICE pointers allocated by the caller; the work is enqueued on `stream` (a hipStream_t, NULL = the null
 * stream) of the current device, asynchronously.  Conventions: particle (i0, i1, i2) of an
 * (N0, N1, N2) lattice sits at q_c = i_c L_c / N_c + psi_c (periodic, scripts/halos.py:394-403), mesh node j at j L_c / res_c,
 * one-dimensional windows are the B-splines of order worder (1 NGP, 2 CIC, 3 TSC, 4 PCS) in units of the mesh spacing. */

/* replaces dj.get_delta_from_psi(psi, method="pm", res, worder, deconvolve=False) (scripts/core.py:449): disp =
 * (3, N0, N1, N2) float32 or float16 (disp_dtype NBE_F32 / NBE_F16); mesh = (res0, res1, res2) int64, ZEROED by the caller,
 * receives the masses in units of 2^-22 particles, bitwise independent of scheduling; every particle adds exactly 2^22.
 * stats = 4 int32 (zeroed by the caller): [0] tiles of 8^3 particles whose footprint took the direct (global-atomic) path,
 * [1] particles with a non-finite or out-of-range position, which are NOT painted, [2:4] one int64: with count_atomics != 0
 * (measurement only: one more same-address atomic per tile) the number of 64-bit atomic adds into the mesh.  A footprint
 * of any accepted size (positions up to 2^30 mesh cells apart on either side) that does not fit the LDS image takes the
 * direct path, here and in the two painters below. */
int nbe_paint_mesh(const void* disp, int disp_dtype, const int64_t n[3], const double boxsize[3], const int64_t res[3],
                   int worder, int count_atomics, void* mesh, void* stats, void* stream);
/* mesh (int64, as above) -> delta = rho / rho_mean - 1 (float32), rho_mean = nparticles / (res0 res1 res2) */
int nbe_mesh_to_delta(const void* mesh, const int64_t res[3], int64_t nparticles, void* delta, void* stream);

/* Per-particle fields: weighted mass assignment in the integer scheme of nbe_paint_mesh.  Channel
 * c of a quantity has the binary exponent e_c with max |q_c| < 2^e_c; particle p carries V_p = rint(q_p 2^(24 - e_c)),
 * |V_p| <= 2^24, and a cell holds S = sum of w V_p (int64, two's complement) over the fixed-point weights w of
 * nbe_paint_mesh.  |S| <= M 2^24 for a cell of mass M units: cells below 2^39 units (2^17 particle masses) cannot overflow. */
#define NBE_PAINT_MAX_CHANNELS 4
#define NBE_FIELD_DENSITY 0
#define NBE_FIELD_MEAN 1
/* first half of project_field_from_particles (scripts/utils.py:151-183, DISCO-DJ compute_field_quantity_from_particles):
 * the range of the quantity.  quantity = (nchan, count) float32 / float16; range = (nchan + 1) uint32, zeroed by the
 * caller: [c] receives the float32 bits of max |q_c| over the finite values, [nchan] the number of non-finite values. */
int nbe_quantity_range(const void* quantity, int dtype, int nchan, int64_t count, void* range, void* stream);
/* replaces the particle-to-mesh step of project_field_from_particles (scripts/utils.py:151-183) and of
 * project_density_slab (scripts/halos.py:468): one read of the particles paints the mass mesh of nbe_paint_mesh (same
 * units, same bits) and nchan quantity meshes.  disp = (3, N0, N1, N2) or NULL (the undisplaced lattice); quantity =
 * (nchan, N0, N1, N2), 0 <= nchan <= NBE_PAINT_MAX_CHANNELS (0: masses only); exponents = nchan host ints e_c.  shift =
 * (N0, N1, N2) or NULL: position along axis shift_axis is i a + psi s + shift * (shift_scale * res / L) in float64
 * (redshift space: shift = the line-of-sight velocity, shift_scale = length per unit of velocity).  mesh = (res) int64,
 * qmesh = (nchan, res) int64, both ZEROED by the caller.  stats = 4 int32, zeroed: [0] tiles on the direct path (footprint
 * beyond the 8192-cell LDS image), [1] particles with a non-finite or out-of-range position, NOT painted; [2] is written
 * by nbe_mesh_to_field. */
int nbe_paint_fields(const void* disp, int disp_dtype, const void* quantity, int quantity_dtype, int nchan,
                     const int exponents[], const void* shift, int shift_dtype, int shift_axis, double shift_scale,
                     const int64_t n[3], const double boxsize[3], const int64_t res[3], int worder, void* mesh,
                     void* qmesh, void* stats, void* stream);
/* Particle catalogues: the integer scheme of nbe_paint_fields for explicit positions.  Replaces
 * nbodykit's catalogue-to-mesh step (ArrayCatalog(...).to_mesh(Nmesh, resampler, position, value).compute(), the way the
 * halos of scripts/halos.py:407-450 reach a mesh) and the particle-to-mesh step of project_field_from_particles for
 * positions that are not a displaced lattice.  pos = (count, 3) row-major, float32 or float64 (pos_dtype NBE_F32 /
 * NBE_F64), any number of boxes away; the mesh coordinate is u_c = x_c (res_c / L_c) in float64, plus shift * (shift_scale
 * * res / L) along shift_axis (shift = (count,) float32 / float16, or NULL).  order = (count,) int64, a permutation of
 * 0 .. count-1, or NULL for the identity: a workgroup paints 512 consecutive entries of it through an 8192-cell LDS image
 * of their footprint, or straight into the meshes where the footprint is larger.  quantity = (nchan, count), exponents,
 * mesh, qmesh and the integers added are those of nbe_paint_fields: the meshes are the same bits for every order.  stats =
 * 4 int32, zeroed: [0] chunks of 512 entries on the direct path, [1] particles with a non-finite or out-of-range position
 * (or an entry of order outside 0 .. count-1), NOT painted; [2] is written by nbe_mesh_to_field.  1 <= count < 2^31. */
int nbe_paint_particles(const void* pos, int pos_dtype, const void* order, const void* quantity, int quantity_dtype,
                        int nchan, const int exponents[], const void* shift, int shift_dtype, int shift_axis,
                        double shift_scale, int64_t count, const double boxsize[3], const int64_t res[3], int worder,
                        void* mesh, void* qmesh, void* stats, void* stream);
/* the order worth passing to nbe_paint_particles (no counterpart in the reference; nbodykit sorts nothing): keys = (count,)
 * int64, keys[p] = the index of the mesh tile of tile_edge^3 cells that holds node floor(u) mod res of particle p (u as
 * above, same shift arguments): row-major over the ceil(res / tile_edge) tiles per axis, or with morton != 0 the
 * interleaved bits of the three tile indices.  A particle nbe_paint_particles would reject gets INT64_MAX.  The caller
 * sorts the keys and passes the permutation as `order`. */
int nbe_particle_keys(const void* pos, int pos_dtype, const void* shift, int shift_dtype, int shift_axis,
                      double shift_scale, int64_t count, const double boxsize[3], const int64_t res[3], int tile_edge,
                      int morton, void* keys, void* stream);
/* Mesh readout, the adjoint of the three painters above, which the reference does not have:
 * stands in for nbodykit's mesh.readout(position, resampler) and Pylians' MASL.CIC_interp.  field = (nchan, res0, res1,
 * res2) float32, 1 <= nchan <= NBE_PAINT_MAX_CHANNELS; out = (nchan, count) float32.  The rows are either a catalogue, pos =
 * (count, 3) float32 / float64 with an optional order, both as in nbe_paint_particles (disp and n are not read), or, with
 * pos = NULL, the lattice n of nbe_paint_fields displaced by disp = (3, N0, N1, N2) float32 / float16 or bare (disp = NULL),
 * count = N0 N1 N2, order = NULL.  With q_abc the fixed-point weights that the painters add for the row (integers that sum
 * to exactly 2^22), out_c = (float)(2^-22 sum of q_abc f_c[node]), summed in float64 in the (a, b, c) order of the weights;
 * q f is exact in float64, so the sum does not depend on fusing.  A row that the painters would not paint (a non-finite
 * position or one beyond 2^30 mesh cells) gets `fill` in every channel and is counted in stats[1]; an entry of order outside
 * 0 .. count-1 names no row: it is counted there too and nothing is written for it.  stats = 4 int32, zeroed by the caller.
 * No atomics on out, one writer per word: the same bits for every order and stream.  out_c(p) = sum over nodes of
 * W(p, node) f_c[node] is the transpose of nbe_paint_particles' mesh = sum over p of W(p, node), with the same integers. */
int nbe_mesh_read(const void* field, int nchan, const int64_t res[3], const void* disp, int disp_dtype, const int64_t n[3],
                  const void* pos, int pos_dtype, const void* order, int64_t count, const double boxsize[3], int worder,
                  double fill, void* out, void* stats, void* stream);
/* second half of project_field_from_particles (normalize_by_density): the meshes of nbe_paint_fields -> field = (nchan,
 * res) float32, in float64 with one rounding.  NBE_FIELD_MEAN: S 2^(e_c - 46) n_cells / nparticles.  NBE_FIELD_DENSITY:
 * S 2^(e_c - 24) / M, and `fill` where M = 0.  stats[2] += the cells with M >= 2^39, whose S may have wrapped. */
int nbe_mesh_to_field(const void* mesh, const void* qmesh, int nchan, const int exponents[], const int64_t res[3],
                      int64_t nparticles, int mode, double fill, void* field, void* stats, void* stream);
/* replaces deconvolve_mas_kernel (scripts/utils.py:136-148): in place on the rfft (res0, res1, res2/2+1) complex64 of a
 * mesh, divide by prod_c sinc(pi f_c / res_c)^worder, sinc(x) = sin(x) / x (the window alone, no alias sum) */
int nbe_deconvolve_mas(void* field, const int64_t res[3], int worder, void* stream);
/* replaces Pk_library.Pk (scripts/utils.py:1083-1085): shell sums over the rfft (n, n, n/2+1) complex64 `a` of an n^3 mesh
 * (b = NULL: |a|^2, else Re(a b*)); shell s = 1 .. n/2 holds the modes with s - 1/2 <= |k| / k_F < s + 1/2, counted over
 * the full grid.  binmax = (n/2+1) uint32, sums = 3 (n/2+1) int64, both zeroed by the caller.  Out: binmax[s] = float bits
 * of the shell's largest |term|; with e_s its binary exponent (binmax = m 2^e_s, m in [0.5, 1)): sums[s] = modes,
 * sums[n/2+1 + s] = sum of (|k| / k_F - s) in units of 2^-36, sums[2 (n/2+1) + s] = sum of the terms in units of
 * 2^(e_s - 32).  Integer sums: reproducible bit for bit.  2 <= n <= 4096. */
int nbe_power_spectrum(const void* a, const void* b, int64_t n, void* binmax, void* sums, void* stream);
/* Anisotropic spectra about the array axis `los` (0 .. 2) of a cubic mesh.  Shells, full-grid
 * weights, terms p = Re(a b*) and binmax are those of nbe_power_spectrum, whose first pass both calls run unchanged; every
 * power sum of shell s is in units of 2^(e_s - 32).  mu^2 = m_los^2 / |m|^2 in float64; only even powers of mu enter, so
 * the half spectrum's missing mirror modes do not matter.  2 <= n <= NBE_PK_ANISO_MAX_N. */
#define NBE_PK_ANISO_MAX_N 2048
#define NBE_PK_MAX_MU 64
/* replaces the multipole columns Pk[:, 0..2] of Pk_library.Pk(delta, boxsize, axis, MAS) (scripts/utils.py:1083-1085,
 * :1447-1449): binmax = (n/2+1) uint32, sums = 5 (n/2+1) int64, both zeroed by the caller.  Out: binmax as
 * nbe_power_spectrum; sums[w (n/2+1) + s] for w = 0 modes, 1 the sum of (|k| / k_F - s) in units of 2^-36, and 2, 3, 4 the
 * sums of rint(p L_l 2^(32 - e_s)) for L_0 = 1, L_2 = (3 mu^2 - 1) / 2, L_4 = (35 mu^4 - 30 mu^2 + 3) / 8 in float64.  Words
 * 0 .. 2 are the bits of nbe_power_spectrum.  The caller applies 2 l + 1 and L^3 / n^6. */
int nbe_power_multipoles(const void* a, const void* b, int64_t n, int los, void* binmax, void* sums, void* stream);
/* replaces the 2-D spectrum Pk2D of Pk_library.Pk(delta, boxsize, axis, MAS) (scripts/utils.py:1083-1085, :1447-1449) with
 * wedges of |mu|: for nmu (1 .. NBE_PK_MAX_MU) bins a mode falls into bin j = min(nmu - 1, #{ j' in 1 .. nmu-1 :
 * j'^2 |m|^2 <= nmu^2 m_los^2 }), that is floor(nmu |mu|) with mu = 1 in the last bin, decided in 64-bit integers.
 * binmax = (n/2+1) uint32, per shell and not per wedge; sums = 4 nmu (n/2+1) int64 laid out [word][mu][s], both zeroed by
 * the caller.  Words: modes, the sum of (|k| / k_F - s) in units of 2^-36, the sum of |mu| = |m_los| / |m| in units of
 * 2^-36, the sum of the terms in units of 2^(e_s - 32).  The mu bins are walked in chunks whose image fits 64 KiB of LDS,
 * one launch each; max_bins (0: that limit) caps the (mu, s) bins of a launch and must hold one mu bin, n/2+1.  Integer
 * sums: the same bits for every chunking. */
int nbe_power_wedges(const void* a, const void* b, int64_t n, int los, int nmu, int max_bins, void* binmax, void* sums,
                     void* stream);

/* Minkowski functionals of an n^3 float32 field, replacing compute_minkowski_functionals and its
 * cubical-complex counting (scripts/utils.py:652-763).  For a threshold t the excursion set is the set M of voxels with
 * w >= t (indices mod n).  Voxel v owns the elements at its low corner: its cube, the face towards v - e_a and the edge
 * along a through v, for each axis a, and its vertex.  Counts: n3 = |M|; n2 = sum over a of #{v : v or v - e_a in M};
 * n1 = sum over a of #{v : v, v - e_b, v - e_c or v - e_b - e_c in M}, {b, c} the other two axes; n0 = #{v : some v - s in
 * M, s in {0,1}^3}.  An element is in the set iff the largest w of its voxels is >= t, so one histogram of element maxima
 * per functional, binned by upper_bound over the sorted thresholds, holds the counts of every threshold at once. */
#define NBE_MF_MAX_N 2048
#define NBE_MF_MAX_THRESHOLDS 1024
#define NBE_MOMENTS_WORDS 2050
/* replaces np.mean / np.std of compute_minkowski_functionals (scripts/utils.py:652-763): the mean and population standard
 * deviation of the field in float64, by two passes (the sum, then the sum of squared deviations from that mean) over a
 * partition of the voxels that depends on n only, reduced in a fixed order: bitwise reproducible.  moments =
 * NBE_MOMENTS_WORDS float64: out [0] mean, [1] std; the rest is scratch.  1 <= n <= NBE_MF_MAX_N. */
int nbe_field_moments(const void* field, int64_t n, void* moments, void* stream);
/* replaces the per-threshold counting loop of compute_minkowski_functionals (scripts/utils.py:652-763): thresholds =
 * nthresholds (T, 1 .. NBE_MF_MAX_THRESHOLDS) float32 sorted ascending; moments = NULL for w = x, else the output of
 * nbe_field_moments, standardizing w = (x - float(mean)) / float(std) (float32, correctly rounded; w = 0 where
 * float(std) = 0).  counts = 4 (T+1) + 1 int64, ZEROED by the caller.  Out: counts[f (T+1) + b] = the elements of kind f
 * (0 vertices, 1 edges, 2 faces, 3 cubes) whose largest bin is b, bin(w) = #{thresholds <= w}; the count of f at sorted
 * threshold k is the sum over b > k.  counts[4 (T+1)] = voxels whose x is not finite (their counts are meaningless).
 * Integer sums: reproducible bit for bit.  1 <= n <= NBE_MF_MAX_N. */
int nbe_minkowski_counts(const void* field, int64_t n, const void* thresholds, int nthresholds, const void* moments,
                         void* counts, void* stream);

/* Reduced bispectrum Q(theta) of an n^3 float32 field by the FFT estimator (Scoccimarro 2000),
 * replacing Pylians' Bk_library.Bk as the reference calls it (scripts/utils.py:1314-1399).  Definition.  Let kappa = k / k_F,
 * k_F = 2 pi / L, let m in Z^3 run over the wave vectors of the full complex grid (each component in (-n/2, n/2]) and let
 * delta_m be the unnormalised forward FFT.
 *   kappa3(theta) = sqrt((kappa2 sin theta)^2 + (kappa2 cos theta + kappa1)^2): theta is the angle between the vectors k1
 *     and k2, so theta = 0 gives kappa1 + kappa2.
 *   Shell S(kappa) = { m != 0 : lo^2 <= |m|^2 < hi^2 }, lo = max(kappa - dk/2, 0), hi = kappa + dk/2; the squares are taken
 *     in float64 and compared with the integer |m|^2.  The DC mode belongs to no shell.
 *   N_tri(theta) = #{ (m1, m2, m3) : m1 in S(kappa1), m2 in S(kappa2), m3 in S(kappa3(theta)), m1 + m2 + m3 = 0 }.
 *   B(theta) = L^6 / n^9 * sum over those triangles of Re(delta_m1 delta_m2 delta_m3) / N_tri(theta).
 *   P_i = L^3 / n^6 * mean of |delta_m|^2 over shell i;  Q(theta) = B / (P1 P2 + P2 P3(theta) + P3(theta) P1).
 * Closure is exact, not modulo n: the caller keeps 2 (kappa1 + kappa2) + 1.5 dk < n.  With F_S = irfftn(delta I_S) the sum
 * over the voxels of F1 F2 F3 is n^-6 times the sum over the triangles; the transforms are the caller's (rocFFT). */
#define NBE_BK_MIN_N 4
#define NBE_BK_MAX_N 2048
#define NBE_BK_MAX_SHELLS 258        /* shell 1, shell 2 and up to 256 third shells */
#define NBE_BK_MAX_EDGES 512
#define NBE_BK_PARTIALS 2048
/* replaces the shell selection of Bk_library.Bk (scripts/utils.py:1314-1399): one pass over the rfft `spectrum`
 * (n, n, n/2+1) complex64 for nshells (1 .. NBE_BK_MAX_SHELLS) shells.  shells = nshells x 4 int64 ON THE DEVICE:
 * lo2 = max(ceil(lo^2), 1), hi2 = ceil(hi^2), koff, kexp.  filtered (or NULL) = nshells spectra of the same shape: shell s
 * receives delta_m where lo2 <= |m|^2 < hi2 and 0 elsewhere (Hermitian, as the bounds are even in m).  binmax = nshells
 * uint32 and sums = nshells x 3 int64, both zeroed by the caller, or both NULL.  Out, as nbe_power_spectrum: binmax[s] =
 * float bits of the shell's largest |delta_m|^2 = m 2^e, m in [0.5, 1); sums[s] = { modes of the full grid, sum of
 * (|m| - koff) in units of 2^-kexp, sum of |delta_m|^2 in units of 2^(e - 32) }.  Integer sums: reproducible bit for bit.
 * NBE_BK_MIN_N <= n <= NBE_BK_MAX_N. */
int nbe_shell_filter(const void* spectrum, int64_t n, const void* shells, int nshells, void* filtered, void* binmax,
                     void* sums, void* stream);
/* replaces the sum over the voxels of the three filtered fields in Bk_library.Bk (scripts/utils.py:1314-1399): out[j] =
 * sum over the n^3 voxels of f1 f2 f3[j] in float64, j < nfields (1 .. NBE_BK_MAX_SHELLS); f3 = nfields contiguous float32
 * fields.  The voxels are partitioned by n alone and every level is added in a fixed order, with no float atomics: out[j]
 * is the same bits on every call, whichever other fields share the call.  partials = nfields x NBE_BK_PARTIALS float64 of
 * scratch, out = nfields float64. */
int nbe_triple_sums(const void* f1, const void* f2, const void* f3, int nfields, int64_t n, void* partials, void* out,
                    void* stream);
/* replaces the triangle counts of Bk_library.Bk (scripts/utils.py:1314-1399), which it takes from transforms of the shell
 * indicators: here every pair of modes1 x modes2 (count x 4 int32: m_x, m_y, m_z, 0) closes with m3 = -(m1 + m2), and
 * |m3|^2 is binned by upper_bound over `edges`, nedges (2 .. NBE_BK_MAX_EDGES) int32 sorted ascending and distinct.
 * hist = nedges + 1 int64, zeroed by the caller: hist[b] = pairs with b = #{edges <= |m3|^2}; a shell [edges[a], edges[c])
 * holds the sum of hist[a+1 .. c].  Integers: exact at every mesh size. */
int nbe_triangle_counts(const void* modes1, int64_t count1, const void* modes2, int64_t count2, const void* edges,
                        int nedges, void* hist, void* stream);

/* One-point statistics of `count` float32 values (any shape; 1 <= count <= 2^40). */
#define NBE_MOMENTS4_WORDS 6148
#define NBE_PDF_MAX_BINS 4096
#define NBE_ONEPOINT_MAX_VOXELS (1LL << 40)
/* replaces _field_moments (scripts/utils.py:1164-1187): moments = NBE_MOMENTS4_WORDS float64: out [0] the mean, [1] the
 * population standard deviation, [2] and [3] the third and fourth central moments (means of (x - mean)^3 and ^4); the
 * rest is scratch.  Float64, two passes over the partition of nbe_field_moments, reduced in a fixed order: bitwise
 * reproducible. */
int nbe_field_moments4(const void* field, int64_t count, void* moments, void* stream);
/* replaces np.histogram(x[isfinite(x)], bins=np.linspace(lo, hi, nbins + 1)) (scripts/utils.py:1248-1274): edges = nbins + 1
 * float64 ascending with edges[0] = lo and edges[nbins] = hi, 2 <= nbins <= NBE_PDF_MAX_BINS.  A value x, widened to
 * float64, falls into bin #{edges <= x} - 1, and x = hi into the last bin (NumPy's rule).  counts = nbins + 2 int64, zeroed
 * by the caller: the bins, then the finite values outside [lo, hi], then the non-finite ones. */
int nbe_field_histogram(const void* field, int64_t count, double lo, double hi, const void* edges, int nbins,
                        void* counts, void* stream);

/* ---- Halos (no context) ------------------------------------------------------------------------------
 * Friends-of-friends groups of the displaced lattice, the step of scripts/halos.py.  Pointers,
 * `stream` and asynchrony as for "Density".  disp = (3, n, n, n) in a cubic periodic box of side boxsize.  Particle
 * p = (i0 n + i1) n + i2 has the integer coordinates X_c = rint((i_c / n + psi_c / L) 2^30) mod 2^30 (float64); the
 * minimum-image difference d_c(p, q) is (X_c(p) - X_c(q)) mod 2^30 in [-2^29, 2^29); p != q are linked iff
 * d_0^2 + d_1^2 + d_2^2 <= r2 in 64-bit integers.  A group is a connected component, labelled by its smallest particle
 * index.  Cells: (X_c ncell) >> 30 per axis, key (c0 ncell + c1) ncell + c2, with 3 <= ncell <= NBE_FOF_MAX_CELLS and
 * ncell (isqrt(r2) + 1) <= 2^30 so that linked particles share a cell or sit in adjacent ones.  max_blocks > 0 caps the
 * grid of a launch (tests); every result is made of integer sums and minima and does not depend on it.  The calls, in
 * order: nbe_fof_cells, the caller's sort of `keys`, nbe_fof_gather, nbe_fof_link, nbe_fof_labels, the caller's choice of
 * halos, nbe_fof_catalog. */
#define NBE_FOF_MIN_N 2
#define NBE_FOF_MAX_N 1024
#define NBE_FOF_MAX_CELLS 4096
/* replaces load_local_positions_from_displacement (scripts/halos.py:359-404): one read of the displacement.  coords =
 * (3, n^3) int32 receives X; keys = n^3 int64 the cell keys; parent = n^3 int32 the identity; stats = 1 int32, zeroed by
 * the caller, counts the particles with a non-finite displacement or |psi_c / L| >= 2^20 (their X and key are 0: the
 * caller must not go on). */
int nbe_fof_cells(const void* disp, int disp_dtype, int64_t n, double boxsize, int ncell, int max_blocks, void* coords,
                  void* keys, void* parent, void* stats, void* stream);
/* the neighbour structure of nbodykit's FOF (scripts/halos.py:407-432, run_fof): order = count int64, the particle
 * indices in ascending order of their keys (ties in any order); sorted = count records of 4 int32 (X_0, X_1, X_2, p) in
 * that order. */
int nbe_fof_gather(const void* coords, const void* order, int64_t count, int max_blocks, void* sorted, void* stream);
/* replaces the FOF(...) run of scripts/halos.py:426-432: sorted as above, sorted_keys = count int64 ascending (the sorted
 * `keys`), parent as nbe_fof_cells left it.  One thread per particle tests each candidate pair of its own and 13 of its
 * neighbour cells once and joins linked pairs in parent[] without locks.  Out: a forest with parent[x] <= x whose trees
 * are the groups and whose roots are the labels. */
int nbe_fof_link(const void* sorted, const void* sorted_keys, int64_t count, int ncell, int64_t r2, int max_blocks,
                 void* parent, void* stream);
/* replaces fof.labels and the Length column of fof_catalog (scripts/halos.py:433-448): parent[x] becomes the label (root)
 * of x; sizes = count int32, zeroed by the caller, receives the group sizes at the labels and 0 elsewhere. */
int nbe_fof_labels(void* parent, int64_t count, int max_blocks, void* sizes, void* stream);
/* replaces the CMPosition / CMVelocity sums of fof_catalog (scripts/halos.py:433-448): slot = count int32, the halo's row
 * at its label and -1 elsewhere.  sums = (rows, 3) int64 without a velocity, (rows, 6) with one, zeroed by the caller:
 * every member x of row s adds d_c(x, label) to sums[s][c] and, with velocity = (3, count) float32 / float16 and
 * exponents e_c (max |v_c| < 2^e_c, nbe_quantity_range), rint(v_c 2^(24 - e_c)) to sums[s][3 + c].  labels = count int32
 * or NULL: receives slot[parent[x]].  wave_reduce != 0 adds runs of one row inside a wave with one atomic: the same
 * integers; the Python caller passes 0, which measured faster. */
int nbe_fof_catalog(const void* coords, const void* parent, const void* slot, const void* velocity, int velocity_dtype,
                    const int exponents[3], int64_t count, int wave_reduce, int max_blocks, void* sums, void* labels,
                    void* stream);

/* ---- Pairs (no context) ------------------------------------------------------------------------------
 * Pair counts of periodic catalogues and the histogram behind xi(r), xi(s, mu) and its multipoles (DESIGN.md section
 * 12.7).  Pointers, `stream` and asynchrony as for "Density"; coordinates, the minimum-image difference d_c, cells and keys
 * as for "Halos", in a cubic periodic box of side L with U = 2^30 units.  A catalogue is (count, 3) positions, any number of
 * boxes away, with X_c = rint((x_c / L) 2^30) mod 2^30 formed in float64 (nbe_pair_coords), or a displaced lattice with the
 * coordinates of nbe_fof_cells.  q = d_0^2 + d_1^2 + d_2^2 in 64-bit integers, always below 2^60.  Radial bins: thresholds
 * T_0 < T_1 < ... < T_nbins, T_b = floor((r_b / L)^2 2^60) (T_0 = -1 for r_0 = 0), and a pair is in bin b iff
 * T_b < q <= T_{b+1}: (r_b, r_{b+1}] on the rounded coordinates, "<= T" being the FoF link rule, so that the auto count
 * for the edges [0, l] is the number of FoF links at linking length l.  mu bins: nmu uniform bins of mu = |d_los| / |d| over
 * [0, 1] about axis los; for q > 0, m = #{ j in 1 .. nmu - 1 : d_los^2 nmu^2 >= j^2 q }, compared as 128-bit products, and
 * m = 0 for q = 0.  An auto count takes each unordered pair {i, j}, i != j, once; a cross count takes every (i in A, j in
 * B), rows that coincide included (q = 0: in the first bin only if T_0 = -1).  Cells: 3 <= ncell <= NBE_FOF_MAX_CELLS with
 * ncell (isqrt(T_nbins) + 1) <= 2^30, so that a counted pair shares a cell or sits in adjacent ones; the cells are found by
 * binary search in the sorted keys, and memory stays O(particles).  Counts are integer sums: the same bits for every launch
 * geometry, sort order of ties and stream.  The calls, per catalogue: nbe_pair_coords or nbe_fof_cells, the caller's sort
 * of `keys`, nbe_fof_gather; then nbe_pair_count. */
#define NBE_PAIR_MAX_BINS 128
#define NBE_PAIR_MAX_MU 32
#define NBE_PAIR_MAX_IMAGE 4096      /* nbins nmu 64-bit counters: a 32 KiB image in LDS */
#define NBE_PAIR_FORM 2               /* nbe_pair_count's form of nbe_pair_count_form: measured fastest (section 12.7) */
/* replaces the positions-to-cells step of Corrfunc's theory.DD / theory.DDsmu (the gridlink of its periodic box) and of
 * nbodykit's SimulationBox2PCF: pos = (count, 3) row-major, float32 or float64 (pos_dtype NBE_F32 / NBE_F64); coords =
 * (3, count) int32 receives X; keys = count int64 the cell keys; stats = 1 int32, zeroed by the caller, counts the rows with
 * a non-finite position or |x_c / L| >= 2^20 (their X and key are 0: the caller must not go on). */
int nbe_pair_coords(const void* pos, int pos_dtype, int64_t count, double boxsize, int ncell, int max_blocks, void* coords,
                    void* keys, void* stats, void* stream);
/* replaces the pair loop of Corrfunc's theory.DD (nmu = 1) and theory.DDsmu (nmu > 1), and the counting step of nbodykit's
 * SimulationBox2PCF: sortedA / keysA = nbe_fof_gather's records and the sorted keys of catalogue A, countA rows; sortedB /
 * keysB / countB those of B, or sortedB = keysB = NULL for the auto count of A.  thresholds = nbins + 1 int64 on the HOST,
 * strictly increasing from -1 or more; 1 <= nbins <= NBE_PAIR_MAX_BINS, 1 <= nmu <= NBE_PAIR_MAX_MU, nbins nmu <=
 * NBE_PAIR_MAX_IMAGE, los in 0 .. 2.  counts = (nbins, nmu) uint64, zeroed by the caller, receives the pairs.  A pair is
 * rejected on |d_c| > isqrt(T_nbins) in 32 bits, binned by a search of the thresholds, added into a per-workgroup LDS image
 * and flushed once with 64-bit atomics.  One thread per row of A walks its cells of B (FoF's decomposition). */
int nbe_pair_count(const void* sortedA, const void* keysA, int64_t countA, const void* sortedB, const void* keysB,
                   int64_t countB, int ncell, const int64_t* thresholds, int nbins, int nmu, int los, int max_blocks,
                   void* counts, void* stream);
/* nbe_pair_count with its two choices made by the caller (tools/time_pairs.py and the tests; the counts are the same bits):
 * form bit 0 adds the equal bins of a wave once instead of one LDS atomic per lane, bit 1 takes one thread per row of A
 * (FoF's decomposition) instead of a workgroup per run of one cell with B in LDS tiles; 0 .. 3. */
int nbe_pair_count_form(const void* sortedA, const void* keysA, int64_t countA, const void* sortedB, const void* keysB,
                        int64_t countB, int ncell, const int64_t* thresholds, int nbins, int nmu, int los, int max_blocks,
                        int form, void* counts, void* stream);

/* ---- Input fields (no context)---------------------------------------------------------------------
 * The reference's pipeline brings a linear density field to the particle grid (resize_density_grid) and turns it into
 * the first-order LPT displacement before process_box (scripts/core.py:302-409).  These are the passes between the
 * caller's transforms.  Pointers, `stream` and asynchrony as for "Density".  A spectrum is torch's
 * row-major half spectrum (n, n, n/2+1) complex64 of an n^3 real field, the unnormalised forward transform; a mode has the
 * integer wave vector m, k = 2 pi m / L, each component in (-n/2, n/2], so an even axis stores its Nyquist row as +n/2.
 * Factors are formed in float64 and every output word is rounded to float32 once.  No atomics: the results do not depend
 * on the launch geometry. */
#define NBE_LPT_MIN_N 2
#define NBE_LPT_MAX_N 2048
/* replaces dj.with_lpt(n_order=1) / dj.evaluate_lpt_psi_at_a(a, n_order=1) (scripts/core.py:396-397): psi_spectrum =
 * (3, n, n, n/2+1) receives psi_c = scale i k_c / |k|^2 delta_k, so that div psi = -scale delta.  psi is 0 at m = 0, and
 * component c is 0 where n is even and |m_c| = n/2: a Nyquist row has no sign, so its derivative is set to zero, which
 * keeps the field real. */
int nbe_zeldovich_spectrum(const void* spectrum, int64_t n, double boxsize, double scale, void* psi_spectrum,
                           void* stream);
/* the divergence of a vector field, which the reference's pipeline does not take (its velocity has no spectral summary;
 * the spectra it would feed are those of scripts/utils.py:1083-1085): spectra = (3, n, n, n/2+1), out = (n, n, n/2+1)
 * receives theta_k = i (2 pi / L) ((m_0 v_0 + m_1 v_1) + m_2 v_2), added in float64 in that order.  Component c is left out
 * where n is even and |m_c| = n/2, as in nbe_zeldovich_spectrum, which keeps the field real.  out must not alias spectra. */
int nbe_divergence_spectrum(const void* spectra, int64_t n, double boxsize, void* out, void* stream);
/* Second-order LPT, which the reference leaves at DISCO-DJ's n_order=1 (scripts/core.py:396-397)
 * although n_order=2 is one argument away.  With nabla^2 phi = delta, nbe_zeldovich_spectrum's psi is -grad phi.  The
 * derivative number of axis c is d_c = m_c, or 0 where n is even and |m_c| = n/2: nbe_zeldovich_spectrum's Nyquist rule,
 * applied once per factor.  The three passes, between the caller's transforms:
 *
 * nbe_lpt2_hessian_spectrum: the Hessian of phi.  Component p of the pair list (0,0), (1,1), (2,2), (0,1), (0,2), (1,2) is
 * phi,ij_k = (double)(d_i d_j) / (double)|m|^2 delta_k with the true integer |m|^2, and 0 at m = 0; it is dimensionless (no
 * box size), and phi,ij = -d_j psi_i holds in the library's own derivative.  out = (count, n, n, n/2+1) receives components
 * first .. first + count - 1, 0 <= first, 1 <= count, first + count <= NBE_LPT2_COMPONENTS: pieces give the bits of the
 * whole, so a caller short of memory makes and transforms them a few at a time.  out must not overlap spectrum.
 *
 * nbe_lpt2_source: hess = (6, n, n, n) float32, the six real fields in the pair order; out = (n, n, n) float32 receives
 * S = ((h0 h1 + h0 h2) + h1 h2) - ((h3^2 + h4^2) + h5^2), the sum of the Hessian's principal 2x2 minors, per voxel in
 * float64 in exactly that order, rounded once.  A product of two float32 is exact in float64, so the result is the bits of
 * that float64 expression whether or not a product is fused into the add after it.  out must not overlap hess.  A
 * grid-stride pass; 16-byte accesses where n^3 is a multiple of 4 and both pointers are 16-byte aligned, 4-byte ones
 * otherwise (component c starts at byte 4 c n^3, so an odd n has no aligned form).
 *
 * nbe_lpt2_spectrum: psi_spectrum = (3, n, n, n/2+1) receives psi_c = i (L / 2 pi) d_c / |m|^2 (scale1 delta_k +
 * scale2 S_k), 0 at m = 0: nbe_zeldovich_spectrum's pass on the sum of two spectra.  With scale1 = a and scale2 =
 * -D_2 / D_1^2 a^2 (3/7 a^2 in an Einstein-de Sitter universe) it is psi^(1) + psi^(2), div psi^(2) = -scale2 S.
 * psi_spectrum must not overlap delta_k or source_k; these two may be the same.
 *
 * max_blocks as for nbe_gaussian_spectrum: <= 0 the default grid, a positive value caps the workgroups (the same bits). */
#define NBE_LPT2_COMPONENTS 6
int nbe_lpt2_hessian_spectrum(const void* spectrum, int64_t n, int first, int count, void* out, int max_blocks,
                              void* stream);
int nbe_lpt2_source(const void* hess, int64_t n, void* out, int max_blocks, void* stream);
int nbe_lpt2_spectrum(const void* delta_k, const void* source_k, int64_t n, double boxsize, double scale1, double scale2,
                      void* psi_spectrum, int max_blocks, void* stream);
/* replaces the "fourier" method of upsample_density_with_discodj (scripts/utils.py:186-234), and is its inverse for
 * n_out < n_in: destination mode m = (n_out / n_in)^3 times the source value at m, where the source value at -m is the
 * conjugate of the stored mirror mode.  n_out > n_in: 0 if any |m_c| > n_in / 2, and a factor 1/2 per axis with
 * 2 |m_c| = n_in (the coarse Nyquist row is split evenly onto +-n_in/2).  n_out < n_in: a destination Nyquist component
 * (2 m_c = n_out) is the sum of the source values at m_c = +n_out/2 and -n_out/2, over all sign combinations of such
 * axes, added in float64.  sphere != 0: modes with 4 |m|^2 > n_in^2 (integers) are 0.  dst must not alias src. */
int nbe_spectrum_resize(const void* src, int64_t n_in, void* dst, int64_t n_out, int sphere, void* stream);
/* replaces _upsample_density_mode_inject_numpy / _jax (scripts/utils.py:261-346, :349-425), n_out >= n_in.  Inside the
 * sphere 4 |m|^2 <= n_in^2: the bits of nbe_spectrum_resize(sphere = 1).  Outside: a Gaussian draw with E|F|^2 = sigma^2,
 * sigma = n_out^3 sqrt(P(|k|) / L^3).  P in float64 from k_table / pk_table (ntable >= 2 float64 ON THE DEVICE, k
 * strictly increasing): linear in k between the points (np.interp), pk_table[0] below them, exp(tail_intercept +
 * tail_slope ln k) above k_table[ntable-1], clamped at 0.  The draw is Philox4x32-10 with key (seed low word, seed high
 * word) and counter (r0, r1, i2, 0), where (r0, r1, i2) is the mode's index in dst; on the planes i2 = 0 and (n_out even)
 * i2 = n_out/2 the rows (i0, i1) and ((n - i0) % n, (n - i1) % n) form a pair, the one with the smaller i0 n + i1
 * supplies the counter and the other takes the complex conjugate.  U1 = (x0 + 1/2) 2^-32, U2 = (x1 + 1/2) 2^-32,
 * g = sqrt(-2 ln U1) (cospi(2 U2) + i sinpi(2 U2)) in float64; F = sigma Re g for a mode that is its own mirror image and
 * sigma g / sqrt(2) otherwise.  dst is the half spectrum of a real field by construction. */
int nbe_spectrum_inject(const void* src, int64_t n_in, void* dst, int64_t n_out, const void* k_table,
                        const void* pk_table, int ntable, double tail_slope, double tail_intercept, double boxsize,
                        uint64_t seed, void* stream);
/* replaces the draw of run_lpt_emulator_pipeline(seed=...) (scripts/core.py:263-302: white noise coloured with a tabulated
 * linear P(k)): dst = (n, n, n/2+1) receives the whole half spectrum of a Gaussian field, Hermitian by construction, one
 * seed being one universe at every n.  Pairing as in nbe_spectrum_inject: on the planes i2 = 0 and
 * (n even) i2 = n/2 the rows (i0, i1) and ((n - i0) % n, (n - i1) % n) form a pair, the one with the smaller i0 n + i1
 * draws, the other takes the complex conjugate, and a row that is its own mirror is a self mode.  Philox4x32-10 with key
 * (seed low word, seed high word) and counter ((uint32) m0, (uint32) m1, (uint32) m2, 1): the two's-complement signed wave
 * numbers of the drawing row, each in (-n/2, n/2], so the counter does not depend on n and never equals one of
 * nbe_spectrum_inject (last word 0).  U1 = (x0 + 1/2) 2^-32, U2 = (x1 + 1/2) 2^-32, g = sqrt(-2 ln U1) (cospi(2 U2) +
 * i sinpi(2 U2)) in float64.  sigma = scale n^3 sqrt(P(|k|) / L^3), multiplied in that order, with P as in
 * nbe_spectrum_inject; F(0) = +0, a self mode gets sigma Re g (imaginary word +0), every other mode sigma g / sqrt(2); each
 * float32 word is rounded once.  Only products follow sigma, so the words at n and 2n differ by exactly 8.
 * flags: NBE_IC_FIXED_AMPLITUDE: a non-self mode gets sigma (cospi(2 U2) + i sinpi(2 U2)), a self mode +sigma if
 * cospi(2 U2) >= 0 and -sigma otherwise.  NBE_IC_INVERT_PHASE: F -> -F for every mode (words that are +0 stay +0).
 * NBE_IC_WHITE_NOISE: sigma = n^(3/2), a real field of unit variance; the table pointers may be NULL and ntable, the tail,
 * boxsize and scale are not read.  max_blocks <= 0: the default grid; a positive value caps the number of workgroups (the
 * same bits: a test makes the row loop wrap on a small mesh with it). */
#define NBE_IC_FIXED_AMPLITUDE 1
#define NBE_IC_INVERT_PHASE 2
#define NBE_IC_WHITE_NOISE 4
int nbe_gaussian_spectrum(void* dst, int64_t n, const void* k_table, const void* pk_table, int ntable,
                          double tail_slope, double tail_intercept, double boxsize, double scale, uint64_t seed, int flags,
                          int max_blocks, void* stream);
/* colours somebody else's white noise as scripts/core.py:263-302 colours its own: in place, spectrum (the half spectrum of
 * a real field w of unit variance) becomes delta_k = w_k scale sqrt(n^3 P(|k|) / L^3), the multiplier in float64, each
 * word of the product rounded once, delta_0 = +0.  P as in nbe_spectrum_inject; scale finite and > 0. */
int nbe_spectrum_colour(void* spectrum, int64_t n, const void* k_table, const void* pk_table, int ntable,
                        double tail_slope, double tail_intercept, double boxsize, double scale, void* stream);
/* replaces Pylians' FT_filter(boxsize, sigma, n, "Gaussian") and field_smoothing (scripts/utils.py:590-591): in place,
 * spectrum *= exp(-|k|^2 sigma^2 / 2) = exp(-2 pi^2 |m|^2 sigma_over_L^2) */
int nbe_gaussian_filter(void* spectrum, int64_t n, double sigma_over_L, void* stream);
/* replaces downsample_density_block_average (scripts/utils.py:531-555): dst (n_out^3 float32) = the mean of each
 * (n_in / n_out)^3 block of src (n_in^3 float32), summed in float64 in a fixed order; n_out divides n_in */
int nbe_block_average(const void* src, int64_t n_in, void* dst, int64_t n_out, void* stream);
/* replaces the "linear" method of upsample_density_with_discodj (scripts/utils.py:186-234): dst (n_out^3 float32) =
 * periodic trilinear interpolation of src (n_in^3 float32) at the nodes i n_in / n_out; n_in divides n_out */
int nbe_trilinear_upsample(const void* src, int64_t n_in, void* dst, int64_t n_out, void* stream);

/* ---- Cosmic web (no context) -----------------------------------------------------------------------------
 * Where in the cosmic web a voxel sits, which the reference's pipeline does not ask: the T-web of
 * Hahn et al. (2007, MNRAS 375, 489) with the free threshold of Forero-Romero et al. (2009, MNRAS 396, 1815) from the tidal
 * tensor phi,ij (nabla^2 phi = delta: nbe_lpt2_hessian_spectrum of the smoothed delta_k), and the V-web of Hoffman et al.
 * (2012, MNRAS 425, 2049) from the velocity shear.  Pointers, `stream`, asynchrony and spectra as for "Input fields";
 * max_blocks as for nbe_lpt2_source (the same bits for every grid).
 *
 * nbe_shear_spectrum: spectra = (3, n, n, n/2+1) of a vector mesh v.  Component p of nbe_lpt2_hessian_spectrum's pair list
 * receives Sigma_ij = -scale (d_i v_j + d_j v_i) / 2 with nbe_divergence_spectrum's derivative i (2 pi / L) d_c, d_c = m_c or
 * 0 on the Nyquist row of an even n; Hoffman et al. have scale = 1 / H0.  Each word is f times the float64 bracket
 * (d_i v_j + d_j v_i) / 2 (exact products, one rounding) with f = -scale 2 pi / L, rounded to float32 once.  The real-space
 * trace is -scale div v.  out = (count, n, n, n/2+1) receives components first .. first + count - 1 as in
 * nbe_lpt2_hessian_spectrum: pieces give the bits of the whole.  out must not overlap spectra.
 *
 * nbe_tensor_eigenvalues: tensor = (6, n, n, n) float32 in the pair order, eig = (3, n, n, n) float32 receives
 * lambda_1 >= lambda_2 >= lambda_3 per voxel: computed in float64 from the six float32 words, sorted, rounded once
 * (csrc/nbe_web.h has the method and its error, far below one float32 rounding of |A|_F).  Where the three off-diagonal
 * words are exactly 0 the result is the sorted diagonal, bit for bit.  A voxel with a non-finite word gives three NaNs.  A
 * grid-stride pass with nbe_lpt2_source's access rule.  eig must not overlap tensor.
 *
 * nbe_web_classify: eig = (3, n, n, n) float32; thresholds = nthresholds finite float32 ON THE HOST, 1 <= nthresholds <=
 * NBE_WEB_MAX_THRESHOLDS (a scan of lambda_th costs one read of eig); counts = (nthresholds, 5) int64, ZEROED by the caller:
 * counts[t][m] += the voxels with exactly m eigenvalues > thresholds[t] in float32 comparison (0 void, 1 sheet, 2 filament,
 * 3 knot), counts[t][4] += the voxels with a NaN eigenvalue, which have no type.  types = (n, n, n) uint8 or NULL: m under
 * thresholds[which], 255 for a NaN voxel.  Sums of ones, reduced per workgroup before the 64-bit atomic. */
#define NBE_WEB_MAX_THRESHOLDS 64
int nbe_shear_spectrum(const void* spectra, int64_t n, double boxsize, double scale, int first, int count, void* out,
                       int max_blocks, void* stream);
int nbe_tensor_eigenvalues(const void* tensor, int64_t n, void* eig, int max_blocks, void* stream);
int nbe_web_classify(const void* eig, int64_t n, const float* thresholds, int nthresholds, int which, void* types,
                     void* counts, int max_blocks, void* stream);

/* ---- Pairwise velocities (no context) ------------------------------------------------------------------
 * Velocity moments per bin of separation: the mean pairwise (streaming) velocity v12(r) and the
 * dispersions sigma_r(r), sigma_t(r) of the streaming model (Peebles 1980; Fisher 1995; Scoccimarro 2004), the
 * pairwise-velocity statistics that go with the counts of Corrfunc's theory module (theory.DD, theory.vpf), and the infall
 * and dispersion profile of matter about halos.  The reference has no such step: it checks its velocity field only through
 * redshift-space positions.  Pointers, `stream` and asynchrony as for "Density"; records, sorted keys, thresholds, the rule
 * T_b < q <= T_{b+1}, ncell and its adjacency condition exactly as for "Pairs", whose code decides every bin.
 *
 * One exponent e per call with max |v_c| < 2^e over all components of all catalogues of the call; W_c = rint(v_c 2^(20 - e)).
 * For a pair (a, o) in a bin: d_c = the minimum-image X_c(o) - X_c(a), dW_c = W_c(o) - W_c(a), u = sum dW_c d_c (int64), the
 * radial word vr = sign(u) floor(|u| / sqrt(q) + 1/2), decided by 128-bit integer comparisons (vr = 0 for q = 0; vr < 0 is
 * approach), and |dW|^2 = sum dW_c^2.  A bin holds six 64-bit words: N, S1 = sum vr, sum (vr^2 & (2^24 - 1)),
 * sum (vr^2 >> 24), and the same two for |dW|^2; vr^2, |dW|^2 < 2^44, so no word overflows below 2^39 pairs a bin.  All are
 * sums of integers fixed by the pair alone: the same bits for every launch geometry, form, row order and stream.  The calls,
 * per catalogue: nbe_pair_coords or nbe_fof_cells, the caller's sort of `keys`, nbe_fof_gather, nbe_velocity_words; then
 * nbe_pair_velocity or nbe_halo_velocity_profiles. */
#define NBE_VELOCITY_BITS 20
#define NBE_VELOCITY_SUMS 6
/* velocity = (count, 3) row-major float32 / float64 (lattice 0; dtype NBE_F32 / NBE_F64) or (3, count) float32 / float16
 * (lattice 1; NBE_F32 / NBE_F16), finite with |v| < 2^exponent (the caller's check: nbe_quantity_range); sorted =
 * nbe_fof_gather's records of the catalogue, whose p is the order of the sort.  words = count records of 4 int32 (W_0, W_1,
 * W_2, 0) receives the words of row sorted[j].p at position j: the word and the gather in one pass. */
int nbe_velocity_words(const void* velocity, int dtype, int lattice, int64_t count, int exponent, const void* sorted,
                       int max_blocks, void* words, void* stream);
/* nbe_pair_count's arguments with nmu = 1 and the velocity records wordsA / wordsB beside the sorted records (sortedB, keysB,
 * wordsB all NULL: the auto count, each unordered pair once -- the terms do not depend on which row is called a).  sums =
 * (nbins, 6) 64-bit words, zeroed by the caller: N (unsigned) and the five sums (two's complement).  One thread per sorted
 * row of A, a per-workgroup LDS image of 6 nbins words flushed once with 64-bit global atomics. */
int nbe_pair_velocity(const void* sortedA, const void* keysA, const void* wordsA, int64_t countA, const void* sortedB,
                      const void* keysB, const void* wordsB, int64_t countB, int ncell, const int64_t* thresholds, int nbins,
                      int max_blocks, void* sums, void* stream);
/* nbe_pair_velocity with its form chosen by the caller (tools/time_pairvel.py and the tests; the same bits): 0 the LDS image,
 * 1 every term added to the global table directly. */
int nbe_pair_velocity_form(const void* sortedA, const void* keysA, const void* wordsA, int64_t countA, const void* sortedB,
                           const void* keysB, const void* wordsB, int64_t countB, int ncell, const int64_t* thresholds,
                           int nbins, int max_blocks, int form, void* sums, void* stream);
/* nbe_halo_profiles's arguments with the velocity records: wordsA those of the centres, or NULL for centres at rest (the
 * matter velocity in the box frame); wordsB those of the matter.  sums = (countA, nbins, 6) int64 row-major, NOT zeroed by
 * the caller: row p (the centre's index before the sort) is written whole with plain stores by the workgroup (form 0) or
 * wave (form 1) that owns it.  The form is chosen as nbe_halo_profiles chooses its own. */
int nbe_halo_velocity_profiles(const void* sortedA, const void* keysA, const void* wordsA, int64_t countA, const void* sortedB,
                               const void* keysB, const void* wordsB, int64_t countB, int ncell, const int64_t* thresholds,
                               int nbins, int max_blocks, void* sums, void* stream);
int nbe_halo_velocity_profiles_form(const void* sortedA, const void* keysA, const void* wordsA, int64_t countA,
                                    const void* sortedB, const void* keysB, const void* wordsB, int64_t countB, int ncell,
                                    const int64_t* thresholds, int nbins, int max_blocks, int form, void* sums, void* stream);

/* ---- Profiles (no context) ---------------------------------------------------------------------------
 * Radial count profiles around centres: one histogram of separations per centre, from which the
 * host forms density profiles and spherical-overdensity radii and masses.  The reference has no such step: its
 * scripts/halos.py stops at the FoF Length, although the Tinker, Tinker10 and Watson fits it overlays (--hmf,
 * scripts/halos.py:203) are defined for spherical-overdensity masses.  Pointers, `stream` and asynchrony as for "Density";
 * records, sorted keys, thresholds, the rule T_b < q <= T_{b+1}, ncell and its adjacency condition exactly as for "Pairs",
 * whose code decides every bin.  The calls, per catalogue (centres A, matter B): nbe_pair_coords or nbe_fof_cells, the
 * caller's sort of `keys`, nbe_fof_gather; then nbe_halo_profiles. */
#define NBE_PROFILE_WAVE_CENTRES 4096 /* nbe_halo_profiles takes form 1 of nbe_halo_profiles_form where countA is at least this */
#define NBE_PROFILE_WAVE_BELOW 3000   /* and 27 countB / ncell^3 is below this, else form 0 (measured, section 12.8) */
/* replaces the profile and spherical-overdensity step of a halo finder such as Rockstar or AHF (the particles about a
 * halo's centre binned in radius), which the reference does not have.  sortedA / keysA = nbe_fof_gather's records and the
 * sorted keys of the centres, countA rows (keysA is part of a catalogue as for nbe_pair_count; this call reads only the
 * records); sortedB / keysB / countB those of the matter.  thresholds = nbins + 1 int64 on the HOST, strictly increasing
 * from -1 or more, 1 <= nbins <= NBE_PAIR_MAX_BINS; counts in 1 .. 2^30; 3 <= ncell <= NBE_FOF_MAX_CELLS with
 * ncell (isqrt(T_nbins) + 1) <= 2^30.  counts = (countA, nbins) uint64 row-major, NOT zeroed by the caller: row p, the
 * centre's index before the sort (the record's p), receives the rows of B in each bin, a row of B that coincides with the
 * centre included (q = 0: in the first bin only if T_0 = -1).  One workgroup of 256 threads per centre, grid-strided
 * (max_blocks > 0 caps the grid), streams the centre's at most 18 ranges of B end to end, adds into an LDS image of 32-bit
 * counters and writes the row with plain stores: no global atomics, and the same bits for every launch geometry.  From
 * NBE_PROFILE_WAVE_CENTRES centres on, where 27 countB / ncell^3 < NBE_PROFILE_WAVE_BELOW, a wave takes a centre instead
 * (form 1 below), which measured faster there. */
int nbe_halo_profiles(const void* sortedA, const void* keysA, int64_t countA, const void* sortedB, const void* keysB,
                      int64_t countB, int ncell, const int64_t* thresholds, int nbins, int max_blocks, void* counts,
                      void* stream);
/* nbe_halo_profiles with its form chosen by the caller (tools/time_profiles.py and the tests; the counts are the same
 * bits): 0 a workgroup per centre, 1 a wave per centre with four centres a workgroup and no workgroup barrier in the loop. */
int nbe_halo_profiles_form(const void* sortedA, const void* keysA, int64_t countA, const void* sortedB, const void* keysB,
                           int64_t countB, int ncell, const int64_t* thresholds, int nbins, int max_blocks, int form,
                           void* counts, void* stream);

/* ---- test / measurement hooks (not part of the reference surface) ------------------------------ */

/* One layer through the production kernels, host NCDHW in / out.  kind: 0 conv3 (VALID 3x3x3),
 * 1 skip (1x1x1, centre-cropped by `crop`), 2 down (k2 s2), 3 up (k2, lhs_dilation 2).
 * flags: 1 = LeakyReLU, 2 = add residual (res/dres shaped like the output).  dx/dw/dy/dres may be NULL. */
int nbe_test_layer(nbe_ctx* ctx, int kind, int crop, int flags, const float* x, const float* dx, int cin,
                   int D, int H, int W, const float* w, const float* dw, const float* bias, int cout,
                   const float* res, const float* dres, float* y, float* dy);
/* The gauged form of a 3x3x3 layer (style_layers_vel.py:98-105 with dW = W (.) (alpha[ci] + beta[co])):
 * dx is the input tangent in this layer's gauge, y = W.x + b, dy = W.dx + beta[o] * (W.x); flags: 1 = LeakyReLU.
 * f16x3 contexts run conv_h3w_kernel (Winograd F(2,3) along z) when the output has an even number of planes, Cin <= 128
 * and NBE_WINO is not 0, else conv_h3g_kernel. */
int nbe_test_layer_gauged(nbe_ctx* ctx, int flags, const float* x, const float* dx, int cin, int D, int H, int W,
                          const float* w, const float* beta, const float* bias, int cout, float* y, float* dy);
/* The same with flags bit 2: res / dres (shaped like the output) are added before the activation -- the float16 model's
 * conv_1 launches, whose Winograd-z form (conv_h3w_kernel<., ., F16>; Cin a multiple of 32) adds the block's skip there.
 * Other precisions run their direct gauged kernels when the residual flag is set. */
int nbe_test_layer_gauged_res(nbe_ctx* ctx, int flags, const float* x, const float* dx, int cin, int D, int H, int W,
                              const float* w, const float* beta, const float* bias, int cout, const float* res,
                              const float* dres, float* y, float* dy);
/* One BLOCK of the loaded, modulated network (style_blocks_vel.py:40-85, :96-166) through the production schedule functions
 * -- the same calls a box makes, so skip fusion, two-source reads, Winograd-z, the hidden tensor's pitch, the narrow tile,
 * the output gauges and the one-launch up-sampling are chosen exactly as in a box.  Host NCDHW float32 in and out.
 *   block      "conv_l00" ... "conv_r01" (residual blocks), "down_l0" ... "down_l2", "up_r2" ... "up_r0"
 *   pad        0: VALID (y and x shrink); 1: periodic-yx -- x, x2, y, h hold interiors, the engine's tensors carry a 1-voxel
 *              wrap-around halo that the hook fills with the schedule's own halo fill
 *   x, dx      (cin, D, H, W); dx = NULL for conv_l00 (the input field has no tangent) and for displacement-only contexts
 *   x2, dx2    decoder blocks conv_r2 / conv_r1 / conv_r00: NULL -> x is the materialised concat([skip, up]) of 2 mid channels;
 *              else x = the skip half and x2 = the up-sampled half, mid channels each, and two_source selects whether the
 *              block reads them as two tensors (the first-slab call of the z-slab schedule: fused blocks, mid a multiple
 *              of 16, of 32 in the float16 model) or from a concat tensor.  up_r*: the skip half (mid, 2D, 2H, 2W) of the concat tensor the layer writes
 *              its result into -- y is then the whole (2 mid) concat tensor; NULL -> a mid-channel tensor of its own (the
 *              two-source form of the z-slab schedule).  Other blocks: NULL.
 *   y, dy      residual blocks (cout, D - 4, H - 4, W - 4) (pad = 1: (cout, D - 4, H, W)); down (mid, D/2, H/2, W/2); up
 *              (mid or 2 mid, 2D, 2H, 2W)
 *   h, dh      residual blocks: the hidden tensor between conv_0 and conv_1, (cmid, D - 2, H - 2, W - 2) (pad = 1: (cmid, D - 2, H, W));
 *              may be NULL
 *   gauges     3 * 2 * mid floats: the tangent gauges of the input [0, 2 mid), the hidden [2 mid, 4 mid) and the output
 *              [4 mid, 6 mid) tensor as the device holds them (zero-filled beyond the tensor's channels, for gauge 0 and
 *              when the context is not gauged).  Tangents cross this call AS STORED: dx + gauge (.) x on the way in, and
 *              likewise dh, dy on the way out; the hook does no gauge arithmetic.
 *   paths      which paths the launches took: see the enum
 * The call's range shift is applied as a box applies it (max(max |x|, max |bias|) -> the power of two, biases scaled) and
 * divided out of what is returned.  The workspace is sized by a dry run; a pending brick is invalidated.  Returns 1 with a
 * message for a block, shape or form it cannot run.  Not to be called between nbe_probe_begin and nbe_probe_end. */
enum { NBE_PATH_SKIP_FUSED = 1,        /* the block's 1x1x1 skip ran inside conv_1                                     */
       NBE_PATH_TWO_SOURCE = 2,        /* conv_0 read concat([x, x2]) from two tensors                                  */
       NBE_PATH_WINO_0 = 4,            /* conv_0 ran the Winograd-z kernel                                              */
       NBE_PATH_WINO_1 = 8,            /* conv_1 ran the Winograd-z kernel                                              */
       NBE_PATH_NARROW = 16,           /* a launch ran on the narrow 16-cout tile                                       */
       NBE_PATH_UP8 = 32,              /* all eight parities of the up-sampling in one launch                           */
       NBE_PATH_SKIP_NODX = 64,        /* the fused skip ran without an input tangent (conv_l00)                        */
       NBE_PATH_TWO_SOURCE_SKIP = 128  /* the fused skip read its input from two tensors                                */ };
int nbe_test_block(nbe_ctx* ctx, const char* block, int pad, int two_source, const float* x, const float* dx, int D, int H, int W,
                   const float* x2, const float* dx2, float* y, float* dy, float* h, float* dh, float* gauges, int* paths);
/* modulation kernel alone: OIDHW weight -> (w_n, dw_tot) */
int nbe_test_modulate(nbe_ctx* ctx, const float* weight, const float* style_weight, const float* style_bias,
                      int cout, int cin, int k, float s0, float s1, float eps, int first_layer,
                      float* w_n, float* dw_tot);

/* Branch probe -- test instrumentation for the kink-aware parity checks (tests/kink.py).
 * The tangent of LeakyReLUVel jumps by a factor 100 at zero (layers_vel.py:184-185), so two float evaluations of the
 * velocity differ wherever a pre-activation is zero to within rounding.  Armed with a block of nout^3 output voxels
 * (origin: coordinates in the output array of nbe_process_box / nbe_process_region / nbe_forward, multiples of 8; the
 * block must lie inside one tile of the plan), the next call records, for every LeakyReLU in the block's dependency cone
 * -- the 23 activation tensors of an (nout + 96)^3 input, core :105-195 -- which branch this library took.  The checker
 * then evaluates the float64 oracle on that cone WITH THESE BRANCHES and requires (a) agreement with the fields at the plain
 * tolerances on every voxel of the block and (b) that the branches differ from the oracle's own only where the oracle's
 * pre-activation is zero to within the tolerance of that tensor.  Works with every schedule (whole tensors, z-slabs,
 * periodic tiles, merged tiles) except brick mode.  hipGraph replay is off while a probe is armed.
 *   nbe_probe_slots    number of activation tensors recorded (23)
 *   nbe_probe_layout   slot i: "block/layer" of the convolution the activation follows, dims = {C, n, nw}: the bits of
 *                      the (C, n, n, n) cone tensor as (C, n, n, nw) 32-bit words, bit b of word w = voxel x = 32 w + b;
 *                      word_offset = its place in the buffer of nbe_probe_read
 *   nbe_probe_read     synchronises, checks that every voxel of every cone tensor was recorded exactly once, copies out */
int nbe_probe_begin(nbe_ctx* ctx, const int64_t origin[3], int nout);
int nbe_probe_slots(nbe_ctx* ctx);
int nbe_probe_layout(nbe_ctx* ctx, int slot, char* name, int name_cap, int dims[3], int64_t* word_offset);
int nbe_probe_read(nbe_ctx* ctx, void* words, int64_t nwords);
int nbe_probe_end(nbe_ctx* ctx);

/* per-kernel HIP-event timing on the engine's stream (bench.py roofline leg) */
int nbe_profile_enable(nbe_ctx* ctx, int on);
int nbe_profile_reset(nbe_ctx* ctx);
int nbe_profile_count(nbe_ctx* ctx);
/* entry i: kernel name, summed device ms, launches, algorithmic FLOPs (2*MAC of valid outputs) */
int nbe_profile_entry(nbe_ctx* ctx, int i, char* name, int name_cap, double* ms, int64_t* launches, double* flops);
/* bytes of device workspace currently held */
int64_t nbe_workspace_bytes(nbe_ctx* ctx);
/* timing-probe builds (-DNBE_DBG=1) only: s_memtime cycle totals per phase of the f16x3 3x3x3 kernel, summed over
 * waves since the last call: [0] prologue; [1]/[4] compute of the two stages of a (chunk, dz) group, [2]/[5] wait for
 * the wave's own DMA, [3]/[6] wait at the barrier; [7] epilogue; [8] number of waves.  Production builds return zeros. */
int nbe_debug_phase_cycles(nbe_ctx* ctx, double* out16);

#ifdef __cplusplus
}
#endif
#endif /* NBE_H */
