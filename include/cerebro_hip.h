/*
 * cerebro_hip.h -- C-ABI of libcerebro_hip.so, the MI355X (gfx950) loop-detection core.
 *
 * The reference (mpkuse/cerebro) has no FFI seam for this path: the dot-product scan is inline in
 * Cerebro::descrip_N__dot__descrip_0_N (src/Cerebro.cpp:903-1103) and the pose verifier is the static C++
 * function StaticTheiaPoseCompute::PNP (src/DlsPnpWithRansac.cpp:132-245).  This header DEFINES the seam
 * at exactly those cut lines; INTEGRATION.md shows the few-line patch a maintainer applies
 * to Cerebro.cpp / DlsPnpWithRansac.cpp to call it.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch/Eigen types.
 *   - every function returns an int status: CHIP_OK (0) or a negative CHIP_ERR_*; nothing throws or aborts
 *     (the reference uses return false / -1 / exit(n); asserts are compiled out in Release, CMakeLists.txt:44).
 *   - the caller owns every in/out buffer; the library owns device memory; nothing is retained after return.
 *   - row index i of the descriptor DB == position i of Cerebro::wholeImageComputedList
 *     (src/Cerebro.cpp:321-326); rows are append-only and never reordered.  Indices are int64 here (the
 *     reference uses int).
 *   - thread safety: one appender thread (desc_th, cerebro_node.cpp:487), one querier thread
 *     (dot_product_th, :499) and one PnP caller (loopcandidate_consumer_th, :509) may use the same ctx
 *     concurrently.  A query only ever reads rows that were fully appended before the call.
 */
#ifndef CEREBRO_HIP_H
#define CEREBRO_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CHIP_ABI_VERSION 7

/* ------------------------------------------------------------------------------------------ status codes */
enum {
    CHIP_OK = 0,
    CHIP_ERR_INVALID_ARG = -1,
    CHIP_ERR_NO_DEVICE = -2,        /* no usable gfx950 device / HIP runtime failure at create            */
    CHIP_ERR_HIP = -3,              /* a HIP runtime call failed; chip_last_hip_error() has the hipError_t */
    CHIP_ERR_OOM = -4,
    CHIP_ERR_NOT_F32 = -5,          /* an appended float64 is not exactly representable as float32        */
    CHIP_ERR_NONFINITE = -6,        /* NaN/Inf in an appended descriptor (Eigen maxCoeff with NaN is unspecified) */
    CHIP_ERR_RANGE = -7,            /* l / k / row index outside the appended range                       */
    CHIP_ERR_UNSUPPORTED = -8,      /* e.g. D not a multiple of 4, topk > CHIP_MAX_TOPK, nq > CHIP_MAX_NQ  */
    CHIP_ERR_TOO_FEW_POINTS = -9,   /* PnP with < 20 correspondences (DlsPnpWithRansac.cpp:136-139 returns -1) */
    CHIP_ERR_BUSY = -10,            /* async slot still in flight / not enqueued                          */
    CHIP_ERR_COMM = -11,            /* an RCCL call failed; chip_last_comm_error() has the ncclResult_t    */
    CHIP_ERR_SHARD_FAILED = -12,    /* a shard of a sharded DB could not take part in this tick / query (e.g. its query rows had
                                       left its ring under a concurrent bulk append); EVERY rank gets this status for that call,
                                       the call had no effect (last_l is not advanced) and the exchange stays in step: retry */
    CHIP_ERR_GROUP_BROKEN = -13     /* an earlier call failed on some devices of a chip_create_multi ctx after they had
                                       diverged (or its communicator failed): the ctx refuses further work -- destroy it */
};

#define CHIP_MAX_TOPK 16
#define CHIP_MAX_NQ 4
#define CHIP_DEFAULT_TOPK 8

typedef struct chip_ctx chip_ctx;

const char *chip_strerror(int status);
int chip_abi_version(void);
/* last hipError_t seen by this ctx (0 = hipSuccess) and its hipGetErrorString text */
int chip_last_hip_error(const chip_ctx *ctx, const char **text);
/* last ncclResult_t seen by this ctx (0 = ncclSuccess) and its ncclGetErrorString text */
int chip_last_comm_error(const chip_ctx *ctx, const char **text);

/* ------------------------------------------------------------------------------------------ lifecycle
 * Replaces  MatrixXd M = MatrixXd::Zero(descriptor_size, 29000)  (src/Cerebro.cpp:946): device-resident,
 * fp32, row-major [row][D], growable (capacity_hint is only the initial reservation; the 29000 ceiling of
 * the reference is not reproduced).
 *
 * Sharding (BASELINE config 4): with shard_count = G > 1 the ctx of rank r stores global rows i with
 * i % G == r (round-robin keeps every prefix [0,k) balanced) plus a replicated ring of the most recent
 * CHIP_RING_ROWS rows (64 MiB at D=4096), from which the tick's three query descriptors are read: a tick at l
 * on a one-process-per-GPU ctx therefore needs chip_db_size() - l <= CHIP_RING_ROWS - 3 (else CHIP_ERR_RANGE /
 * CHIP_ERR_SHARD_FAILED) -- always true in live operation, where ticks trail the append head by a few rows; a
 * chip_create_multi ctx has no such limit (older query rows are fetched from the devices that own them, so a whole
 * recorded schedule can be replayed over a cold-started DB).  Every rank must be fed the same append
 * stream.  One process per GPU; the per-shard top-k lists are exchanged INSIDE the library once an RCCL
 * communicator is attached (chip_comm_init_rank below), or by the HOST (any transport) between
 * chip_scan_local and chip_merge_decide.  Query rows of chip_query_rows / chip_query_scores: with an exchange
 * attached (or on a chip_create_multi ctx) ANY appended row -- it is fetched from the shard that owns it; on a
 * sharded ctx without an exchange only rows still in this rank's ring (else CHIP_ERR_RANGE).                */
#define CHIP_RING_ROWS 4096
int  chip_create(chip_ctx **out, int32_t D, int64_t capacity_hint, int32_t device, int32_t shard_rank, int32_t shard_count);
void chip_destroy(chip_ctx *ctx);

/* Storage type of the DB rows.  The reference's M is MatrixXd (src/Cerebro.cpp:946); the default NetVLAD server emits
 * float32 VALUES on the float64 wire (whole_image_desc_compute_server.py:631,648), for which float rows are lossless and
 * half the HBM traffic; the ReljaNetVLAD model (:148-149, numpy matmul with the WPCA matrix, the only 4096-D model) emits
 * genuine float64, for which the rows must be double to keep the candidate selection bit-exact.
 *   chip_create / flags 0 : decided by the data -- float rows, unless the FIRST append (into the still empty DB) carries a
 *                           value that is not float32-representable: then the DB becomes a double-row DB and that append
 *                           succeeds unrounded.  Later non-representable values in a float DB fail (CHIP_ERR_NOT_F32).
 *   CHIP_CREATE_STORE_F32 : float rows, never switches.        CHIP_CREATE_STORE_F64 : double rows from the start.
 * Double rows: scores are fp64 FMA chains (one rounding per term) in the fixed order of DESIGN.md 3 with 2 elements per lane
 * per 128-element chunk; D <= 10 240 as for float rows (two double queries fit the 160 KiB of LDS; where the three of a
 * tick do not -- D > 6824, e.g. the reference's default 8192 -- the rest is read in place, same bits); the MFMA many-query
 * mode reads double rows only through chip_query_batch_cast_f32 (rows narrowed to float in the loader, opt-in).          */
#define CHIP_CREATE_STORE_F32 1u
#define CHIP_CREATE_STORE_F64 2u
int  chip_create_ex(chip_ctx **out, int32_t D, int64_t capacity_hint, int32_t device, int32_t shard_rank, int32_t shard_count,
                    uint32_t flags);

/* ------------------------------------------------------------------------------------------ multi-GPU inside the library
 * (a) ONE process, G GPUs -- the shape of the reference: the loop-candidate producer is one thread of one process
 *     (src/cerebro_node.cpp:499, src/Cerebro.cpp:903).  chip_create_multi returns ONE ctx backed by G per-device
 *     sub-contexts (rows round-robin, row i on devices[i % G]).  The entry points of the reference's path work on it
 *     unchanged: chip_db_append_* (every device is SENT only the rows it owns plus the newest CHIP_RING_ROWS of the batch: a
 *     bulk load moves ~1x the batch over PCIe, not Gx; the validation decision is one, from all devices),
 *     chip_db_read_rows_*, chip_loop_tick* = G local scans -> per-device local top-k -> exchange -> merge + decision on
 *     devices[0], chip_query_rows / _vectors_* / _scores, chip_synchronize, chip_profile_*, PnP / ICP (on devices[0]).
 *     chip_query_batch_f32 (the MFMA many-query mode: one pass per device over its rows, the per-device lists merged on devices[0]).
 *     NOT on a group ctx (CHIP_ERR_UNSUPPORTED): chip_set_stream / chip_reset_stream, chip_scan_local, chip_merge_decide*,
 *     chip_comm_init_rank (the group owns its exchange).
 *     One host worker thread per device enqueues that device's work, so the host cost of a tick does not grow with G.
 *     Failure containment: a call that fails on SOME devices before anything became visible changes nothing; a shard that
 *     cannot take part in one tick sends a marked neutral list, the tick fails everywhere alike (CHIP_ERR_SHARD_FAILED) and the
 *     exchange stays in step; a failure after the devices diverged marks the ctx broken (CHIP_ERR_GROUP_BROKEN).
 *     Exchange: an RCCL communicator over the G devices (ncclCommInitAll; ncclAllGather of 3 x topk (score,index) entries per
 *     rank per tick, enqueued in-stream between the local and the global merge) when the devices are distinct; device
 *     copies (lists written / copied straight into the root's gather buffer behind events) when CHIP_MULTI_EXCHANGE_COPY is
 *     passed or the list names a device twice (RCCL refuses two ranks on one device) -- the latter lets a 1-GPU box run the
 *     G = 2..8 code path.  RCCL is loaded with dlopen (librccl.so.1, or $CHIP_RCCL_LIBRARY), the library does not link it: if it
 *     is absent, cannot build the communicator, or its bootstrap does not return within CHIP_COMM_INIT_TIMEOUT_MS (default
 *     120 s; the blocking rendezvous runs on a helper thread and is abandoned at the deadline) the create neither fails nor
 *     hangs, it falls back to the copy exchange (chip_get_info().exchange / .comm_ranks / .comm_init_abandoned tell which one
 *     is in use, over how many ranks, and whether a helper is still stuck; chip_last_comm_error() why).  chip_comm_init_rank
 *     has the same deadline: it returns CHIP_ERR_COMM instead of hanging.
 * (b) one process PER GPU (torchrun-style launch): create each rank's ctx with chip_create(.., shard_rank, shard_count),
 *     then attach an RCCL communicator: rank 0 calls chip_comm_unique_id, distributes the 128 bytes by any means, every
 *     rank calls chip_comm_init_rank.  From then on chip_loop_tick / _enqueue / _collect and chip_query_* work on the
 *     sharded ctx (collectively: every rank must make the same calls in the same order) and return the same result on
 *     every rank.  chip_scan_local / chip_merge_decide remain for callers that bring their own transport.          */
#define CHIP_MULTI_EXCHANGE_COPY 4u
int  chip_create_multi(chip_ctx **out, int32_t D, int64_t capacity_hint, const int32_t *devices, int32_t n_devices, uint32_t flags);
#define CHIP_COMM_ID_BYTES 128
int  chip_comm_unique_id(void *id_out /* CHIP_COMM_ID_BYTES */);
int  chip_comm_init_rank(chip_ctx *ctx, const void *id /* CHIP_COMM_ID_BYTES */, int32_t n_ranks, int32_t rank);
/* Make an externally owned hipStream_t (e.g. the stream torch.distributed synchronises its collectives with) the
 * ctx stream: synchronous queries, merges and the stream-ordering promises of chip_scan_local refer to it.  The value
 * is taken literally: NULL is HIP's null stream.  chip_reset_stream returns to the ctx's private stream. */
int  chip_set_stream(chip_ctx *ctx, void *hip_stream);
int  chip_reset_stream(chip_ctx *ctx);
int  chip_synchronize(chip_ctx *ctx);

/* ------------------------------------------------------------------------------------------ DB append
 * Replaces  M.col(_s) = ...getWholeImageDescriptor()  (src/Cerebro.cpp:1005-1006) and the f64 wire type of
 * WholeImageDescriptorCompute.srv:4 / Cerebro.cpp:268-271.  n descriptors, each D contiguous values.
 * The f64->f32 narrowing is done on the device and VERIFIED lossless ((double)(float)x == x); the default
 * NetVLAD server emits float32 values (whole_image_desc_compute_server.py:631,648) so this holds.
 * On CHIP_ERR_NOT_F32 / CHIP_ERR_NONFINITE nothing is appended.                                         */
#define CHIP_APPEND_ALLOW_ROUNDING 1u   /* the caller vouches that the values ARE float32 descriptors up to the precision they were
                                           printed / transmitted with (a state.json checkpoint: 15-digit text): round to nearest
                                           instead of failing -- also in an empty undecided DB, which then stays a float DB; sets
                                           info.lossy_rows.  Without the flag the data decides (chip_create above).  The flag
                                           never stores an Inf: a finite value whose nearest float32 is +-Inf (|x| >= 0x1.ffffffp+127)
                                           is CHIP_ERR_NONFINITE with it (without it CHIP_ERR_NOT_F32, or double rows, as before).  */
int chip_db_append_f64(chip_ctx *ctx, const double *desc, int64_t n, uint32_t flags, int64_t *first_index);
int chip_db_append_f32(chip_ctx *ctx, const float *desc, int64_t n, int64_t *first_index);
int64_t chip_db_size(const chip_ctx *ctx);           /* global number of appended rows (== l)             */
/* Read back rows (global indices; in sharded mode only rows owned by this rank or still in the ring). */
int chip_db_read_rows_f32(chip_ctx *ctx, const int64_t *rows, int64_t n, float *out);   /* CHIP_ERR_NOT_F32 on a double-row DB */
int chip_db_read_rows_f64(chip_ctx *ctx, const int64_t *rows, int64_t n, double *out);

/* Bench/test helper: append n rows of the integer-domain synthetic generator generated ON DEVICE
 * (spec: oracle/dot_scan.c orc_synth_row_f32; SURVEY.md 8d allows on-device generation for the 1M DB).
 * plant_* (may be NULL) list planted rows as GLOBAL row indices inside the appended range, sorted by dst:
 * kind 1 = noisy copy of src (cos ~ 0.98), kind 2 = exact duplicate of src.                            */
int chip_db_append_synthetic(chip_ctx *ctx, int64_t n, uint64_t seed,
                             const int64_t *plant_dst, const int64_t *plant_src, const int32_t *plant_kind, int64_t n_plant);
/* Same rows normalised to UNIT L2 norm (ABI 7; SURVEY.md 8d: "rows = unit-L2-norm", what NetVLAD's last layer emits): the row's integers
 * v_e, S = sum v_e^2 exactly in 64-bit integers, element = (float)((double)v_e * (1 / sqrt((double)S))) -- every floating-point step one
 * correctly rounded operation, so the device rows equal oracle/dot_scan.c orc_synth_row_unit_f32 bit for bit.  Planted rows: kind 1 is the
 * unit vector along 5 src + own (cos ~ 0.98 with src), kind 2 the unit vector of src.  bench.py's headline database is made by this call. */
int chip_db_append_synthetic_unit(chip_ctx *ctx, int64_t n, uint64_t seed,
                                  const int64_t *plant_dst, const int64_t *plant_src, const int32_t *plant_kind, int64_t n_plant);

/* ------------------------------------------------------------------------------------------ descriptor projection
 * (ABI 7, additive.)  For the reference's one 4096-D model, ReljaNetVLAD, the descriptor is not what the network emits: the server
 * takes the 32768-D float32 VLAD vector and applies the whitening PCA and an L2 normalisation on a host core
 * (scripts/whole_image_desc_compute_server.py:145-149), a 32768 x 4096 matrix streamed through a CPU for every keyframe.  These
 * entries keep that matrix on the device and make the row there: z = (Mt x + b) / |Mt x + b|, appended without a host round trip.
 *
 * The definition.  Inputs: x, in_dim float32 values (what model.predict returns); Mt, D x in_dim, one contiguous row per OUTPUT
 * component, Mt[j][i] = WPCA_M[i][j], i.e. np.ascontiguousarray(WPCA_M.T), of element type CHIP_PROJ_F32 or CHIP_PROJ_F64; b, D
 * doubles or NULL; D the ctx's descriptor size.
 *   - CHIP_PROJ_F32:  t_j = orc_dot_tree_f32(x, Mt[j], in_dim): lane L of 64 accumulates elements k*256 + 4L + c (k ascending,
 *     c = 0..3) by fma into one fp64 accumulator -- the products of two float32 values are exact in fp64 -- then the xor butterfly
 *     acc[L] += acc[L ^ m], m = 32..1.
 *   - CHIP_PROJ_F64:  t_j = orc_dot_tree_f64((double)x, Mt[j], in_dim): elements k*128 + 2L + c (c = 0, 1), ONE fused multiply-add
 *     per term (its single rounding is part of the definition), the same butterfly.
 *     These are exactly the orders of DESIGN.md 3 for DB rows of that type: y = Mt x is the score vector of one query against a
 *     database of D rows of in_dim elements.
 *   - y_j = t_j + b_j, one IEEE addition; with b == NULL y_j = t_j and nothing is added.
 *   - s = orc_dot_tree_f64(y, y, D);  r = sqrt(s), correctly rounded;  z_j = y_j / r, IEEE division.  The row is z.
 *   - Nothing is special-cased: r == 0 gives NaN, a NaN or Inf anywhere in x, Mt or b reaches z, and the append's own check
 *     refuses the row (CHIP_ERR_NONFINITE).
 *   - Limits: in_dim % 256 == 0, 256 <= in_dim <= CHIP_PROJ_MAX_IN_DIM (x stays in the LDS as float32: 128 of its 160 KiB); any
 *     D a ctx accepts.
 * UNPINNED against numpy: np.matmul sums in the order of whatever BLAS numpy was built with (float32 sgemv if both operands are
 * float32), np.linalg.norm likewise, and the dtype of the reference's .mat files is on no machine of this project.  What the tests
 * prove is device == this definition, bit for bit, and that the definition lies within the standard gamma bound of the exact
 * rational result.
 *
 *   - chip_project_set uploads the matrix once (in_dim * D * 4 or * 8 bytes of device memory, the bias next to it as doubles); it
 *     lives until chip_project_clear or chip_destroy.  A second call replaces the projection; the new matrix is complete on the device
 *     before the old one goes, so both exist for the duration of the call and CHIP_ERR_OOM leaves the earlier projection in place.
 *   - chip_project_info: in_dim 0 and matrix_type 0 when none is set; any output pointer may be NULL.
 *   - chip_project: the definition made callable (the reference also keeps the descriptor in its DataNode and its state.json):
 *     n raw descriptors -> z, n x D doubles in host memory.  One pass over the matrix per descriptor, or per group of descriptors
 *     where n > 1 ("batched ingest" below): the same bits either way.
 *   - chip_db_append_projected_f32 is chip_db_append_f64 with the rows made on the device: every rule of that call holds (validation,
 *     the storage type decided by an empty undecided DB -- which becomes a double-row DB --, CHIP_ERR_NOT_F32 on a float-row DB with
 *     nothing appended, CHIP_APPEND_ALLOW_ROUNDING, lossy_rows, row_norm_max, publication when the rows are resident), and the DB
 *     afterwards is indistinguishable from chip_db_append_f64(ctx, z of chip_project, n, flags, ..).
 *   - x may be host memory, or device memory of the ctx's device (e.g. the data_ptr() of a torch tensor when the backbone runs
 *     under PyTorch-ROCm in the same process): it is copied with hipMemcpyDefault on the append stream, and the CALLER vouches
 *     that x is complete -- whatever produced it on another stream has been waited for.
 *   - These calls are appends: they serialise with chip_db_append_* of the ctx and may run beside its queries and ticks.  With
 *     CHIP_TICK_RESIDENT=1, chip_project and chip_db_append_projected_f32 pause the resident scan instance for their duration (as
 *     chip_resident_pause does: ticks that arrive meanwhile are launched, the next one afterwards starts a new instance): project_rows
 *     needs a workgroup with up to 128 KiB of LDS on every CU, which cannot be placed beside the instance's.
 * Status, in this order: a NULL ctx / Mt / x / z or n < 0 CHIP_ERR_INVALID_ARG; in_dim outside the limits or an unknown matrix_type
 * CHIP_ERR_UNSUPPORTED (both before the ctx is touched); a chip_create_multi ctx or a sharded ctx (shard_count > 1)
 * CHIP_ERR_UNSUPPORTED; no projection set CHIP_ERR_BUSY; n == 0 CHIP_OK (first_index is filled).                              */
#define CHIP_PROJ_F32 1
#define CHIP_PROJ_F64 2
#define CHIP_PROJ_MAX_IN_DIM 32768
int chip_build_has_project(void);          /* 1 */
int chip_project_set(chip_ctx *ctx, int32_t in_dim, const void *Mt, int32_t matrix_type, const double *bias /* may be NULL */);
int chip_project_clear(chip_ctx *ctx);
int chip_project_info(const chip_ctx *ctx, int32_t *in_dim, int32_t *matrix_type, int32_t *has_bias);
int chip_project(chip_ctx *ctx, const float *x, int64_t n, double *z /* n x D, host */);
int chip_db_append_projected_f32(chip_ctx *ctx, const float *x, int64_t n, uint32_t flags, int64_t *first_index);

/* ------------------------------------------------------------------------------------------ NetVLAD pooling
 * (ABI 7, additive.)  The one non-stock layer of both of the reference's models is its custom Keras layer NetVLADLayer / GhostVLADLayer
 * (scripts/predict_utils.py:11-64, 83-141): NetVLADImageDescriptor = MobileNet conv_pw_7_relu, K = 16, 8192-D, the default
 * (whole_image_desc_compute_server.py:206-218); ReljaNetVLAD = VGG16 block5_pool, K = 64, 32768-D, then the projection above.  These
 * entries take the trunk's last feature map and make the pooled vector -- and the DB row -- on the device: map -> v -> row, or
 * map -> v -> projection -> row, without a host round trip.  The CNN trunk itself stays the producer's.
 *
 * The definition.  THIS PROJECT'S OWN: IEEE fp64 basic operations in stated orders, nothing fused unless it says orc_dot_tree_*; the
 * device reproduces it bit for bit (tests/np_mirror_vlad.py restates it).  UNPINNED against Keras/TF: a TF build's convolution, softmax,
 * exp and reduction orders are not a definition and no TF exists on any machine of this project (DESIGN.md 6 lists the departures).
 * Inputs: x, N positions x C channels of float32, n = row * W + col; Wt, (K+G) x C float32, one contiguous row per cluster
 * (kernel[0,0].T); bias, K+G float32; centres, K x C float32 (C[0,0,0].T, the first K rows), which the layer ADDS, as the reference
 * does (predict_utils.py:48).  K kept clusters, G ghost clusters (0 for NetVLADLayer).
 *   1. Scores, k < K+G:  s[n][k] = orc_dot_tree_f32(x[n], Wt[k], C) + (double)bias[k]: lane L of 64 accumulates elements
 *      j*256 + 4L + c (j ascending, c = 0..3; elements past C are skipped) by fma -- the products are exact in fp64 --, then the xor
 *      butterfly acc[L] += acc[L ^ m], m = 32..1; then one IEEE addition.  (The score vector of one query against a DB of K+G rows.)
 *   2. Softmax:  m = s[n][0]; for k = 1..: if (s[n][k] > m) m = s[n][k];  e_k = vlad_exp(s[n][k] - m);  Z = ((0.0 + e_0) + e_1) + ...
 *      ascending;  a[n][k] = e_k / Z, IEEE division.
 *   3. vlad_exp(t), t <= 0:  t < -700.0 gives +0.0.  Otherwise kf = rint(t * LOG2E), ties to even;
 *      r = (t - kf * LN2_HI) - kf * LN2_LO;  p = c_13; for i = 12..0: p = p * r + c_i, each * and + rounded;  the result is p * 2^kf,
 *      an exact scaling (kf >= -1010: the power, built from its bit pattern, and the result are normal).
 *      LOG2E = 0x1.71547652b82fep+0, LN2_HI = 0x1.62e42fee00000p-1, LN2_LO = 0x1.a39ef35793c76p-33, c_i = 1.0 / (double)i! (the double
 *      nearest 1/i! for i <= 13).  Within 2 ulp of exp on [-700, 0] (1.08 measured), vlad_exp(0) == 1.0.
 *   4. Aggregation in blocks of CHIP_VLAD_BLOCK = 64 positions -- part of the definition, independent of grid and device.  Block j holds
 *      positions 64j .. min(64j + 63, N - 1).  For k < K only (ghost rows are never formed):  P_j[k][c] is the ascending chain over
 *      the block's n, from 0.0, of acc = acc + (a[n][k] * (double)x[n][c]), product rounded, sum rounded;  S_j[k] the ascending chain
 *      of acc + a[n][k];  V[k][c] and A[k] the ascending chains over j of P_j and S_j, from 0.0.
 *   5. Centres:  Wv[k][c] = V[k][c] + (A[k] * (double)centres[k][c]) -- the factored form of sum a (x + C), a stated departure from
 *      the reference's per-term float32 sum.
 *   6. Intra-normalisation:  q_k = orc_dot_tree_f64(Wv[k], Wv[k], C) (lane L: elements j*128 + 2L + c, c = 0, 1, one fma per term, the
 *      same butterfly);  r_k = sqrt(q_k > 1e-12 ? q_k : 1e-12) (Keras' l2_normalize epsilon);  U[k][c] = Wv[k][c] / r_k.
 *   7. q = orc_dot_tree_f64(U, U, K*C) over the k-major flattening;  r = sqrt(q > 1e-12 ? q : 1e-12);
 *      v[k*C + c] = (float)(U[k][c] / r), rounded to nearest even.  The pooled vector is float32, as the Keras layer's output is.
 * Non-finite values: chip_vlad_set refuses a NaN or Inf in Wt, bias or centres (a host check, CHIP_ERR_NONFINITE).  A non-finite score
 * s[n][k] -- which every NaN or Inf of the map produces -- makes the call return CHIP_ERR_NONFINITE with nothing appended and v
 * unspecified.  Everything else is finite by construction: an all-zero map with zero centres gives an all-zero vector through the
 * epsilon, and it is appended like any finite row.
 * Limits: C % 4 == 0, 4 <= C <= 1024; K >= 1, G >= 0, K + G <= 128; (K+G) * C <= 32768; K * C <= CHIP_PROJ_MAX_IN_DIM;
 * 1 <= positions <= CHIP_VLAD_MAX_POSITIONS.
 *
 *   - chip_vlad_set uploads the weights once; they live until chip_vlad_clear or chip_destroy.  A second call replaces them only once
 *     the new ones are complete on the device (as chip_project_set).  chip_vlad_info: all 0 when none are set; pointers may be NULL.
 *   - chip_vlad: the definition made callable, one map -> v, K*C floats in host memory.
 *   - chip_db_append_vlad_f32 appends ONE row made from one map.  With a projection set, its in_dim must equal K*C: the kernels write v
 *     where chip_db_append_projected_f32 stages its input and the call goes on as that one, so the row is indistinguishable from
 *     chip_db_append_projected_f32(v of chip_vlad).  With none set, K*C must equal D, and the row is indistinguishable from
 *     chip_db_append_f64((double)v of chip_vlad): every rule of that call holds (storage decision, row_norm_max, publication); a float32
 *     value always passes the float-row check.
 *   - fmap may be host memory or memory of the ctx's device (a torch tensor's data_ptr(): CHIP_VLAD_NCHW is what a torch trunk emits
 *     for a batch of one): copied with hipMemcpyDefault on the append stream, the CALLER vouches that the map is complete.
 *   - chip_debug_vlad_stage: a (N x (K+G)), V (K x C), A (K) of the ctx's last pooling call, any pointer may be NULL; it launches nothing.
 *   - These calls are appends (they serialise with chip_db_append_*).  With CHIP_TICK_RESIDENT=1 chip_vlad and chip_db_append_vlad_f32
 *     pause the resident scan instance for their duration, as chip_project does.
 * Status, in this order: a NULL ctx / array CHIP_ERR_INVALID_ARG; the limits or an unknown layout CHIP_ERR_UNSUPPORTED (both before
 * the ctx is touched); a chip_create_multi or sharded ctx CHIP_ERR_UNSUPPORTED; chip_vlad_set: a non-finite weight
 * CHIP_ERR_NONFINITE; no weights set CHIP_ERR_BUSY (chip_debug_vlad_stage: also no pooling call yet); K*C against D / in_dim
 * CHIP_ERR_UNSUPPORTED.                                                                                                         */
#define CHIP_VLAD_NHWC 1   /* x[n][c]: Keras channels_last                      */
#define CHIP_VLAD_NCHW 2   /* x[c][n]: what a torch trunk emits (batch of one)  */
#define CHIP_VLAD_BLOCK 64
#define CHIP_VLAD_MAX_POSITIONS 16384
int chip_build_has_vlad(void);             /* 1 */
int chip_vlad_set(chip_ctx *ctx, int32_t channels, int32_t clusters, int32_t ghost, const float *Wt, const float *bias, const float *centres);
int chip_vlad_clear(chip_ctx *ctx);
int chip_vlad_info(const chip_ctx *ctx, int32_t *channels, int32_t *clusters, int32_t *ghost);
int chip_vlad(chip_ctx *ctx, const float *fmap, int32_t positions, int32_t layout, float *v /* clusters*channels, host */);
int chip_db_append_vlad_f32(chip_ctx *ctx, const float *fmap, int32_t positions, int32_t layout, uint32_t flags, int64_t *first_index);
int chip_debug_vlad_stage(chip_ctx *ctx, double *a /* N x (K+G) */, double *V /* K x C */, double *A /* K */);

/* ------------------------------------------------------------------------------------------ batched ingest
 * (ABI 7, additive.)  The two sections above make one DB row per call.  A map rebuilt from a recorded run, a server that takes keyframes
 * from several agents, a trunk that runs at batch B hand over many at once; these entries take them in one call.  Nothing of the
 * definitions changes: every row has the bits the single call gives for it.
 *
 * Several descriptors per pass over the matrix.  chip_project and chip_db_append_projected_f32 with n > 1 walk their descriptors in
 * groups of `width`; a group shares ONE pass over the matrix (kernel project_pass: per output row and descriptor the accumulation order of
 * the definition, so the bits of n single calls), a group of one is the single launch it always was.  The matrix is read
 * ceil(n / width) times instead of n (per staging-sized chunk of rows, 64 MiB of doubles, where n is larger than that).
 *   - chip_project_plan: what a call over n descriptors launches, without a ctx or a device, from the function the launch sizes itself
 *     with: width; passes = ceil(n / width) reads of the matrix, of which shared_passes are project_pass launches and single_launches
 *     (0 or 1: a trailing group of one; n == 1) the single kernel; slab, the elements of x per descriptor the shared pass keeps in the LDS
 *     at a time (twice over: the next slab is loaded while this one is used), a whole number of 1-KiB chunks of a matrix row;
 *     lds_bytes and block of the shared pass; single_lds_bytes of the single launch.  A NULL out or n < 0 CHIP_ERR_INVALID_ARG; in_dim
 *     or matrix_type outside chip_project_set's limits CHIP_ERR_UNSUPPORTED.
 *   - chip_debug_project_last: what the ctx's last projecting call (chip_project, chip_db_append_projected_f32, a pooled append through
 *     a projection) launched, counted apart: passes[0] shared passes and passes[1] single launches, descriptors[0] and descriptors[1] the
 *     descriptors each kind served; width as chip_project_plan has it.  Any pointer may be NULL.  A call that was run twice (an empty
 *     undecided DB that became a double-row DB) reports its second run.
 *
 * Several maps per call.  Map m starts at fmaps + m * positions * C, each in `layout`: a torch [B, H, W, C] (CHIP_VLAD_NHWC) or
 * [B, C, H, W] (CHIP_VLAD_NCHW) tensor's data_ptr(), or host memory.
 *   - chip_vlad_batch: row m of v is chip_vlad(map m), n_maps x K*C floats in host memory.
 *   - chip_db_append_vlad_batch_f32 is ONE append of n_maps rows: row m is byte for byte what chip_db_append_vlad_f32(map m) would
 *     have appended at that place, directly or through the projection -- there the pooled vectors of a group go where
 *     chip_db_append_projected_f32 stages its input, and share the matrix passes above.  Every rule of the single calls holds
 *     (CHIP_APPEND_ALLOW_ROUNDING, the storage-type decision, row_norm_max, lossy_rows, publication when all rows are resident, the pause
 *     of the resident scan instance).  A non-finite score in ANY map refuses the whole call with CHIP_ERR_NONFINITE: nothing is appended,
 *     v is not written.
 *   - The library walks the maps in groups: as many maps as keep the group's positions <= 32768, at least 1 and at most 16; its scratch
 *     is sized for one group, and a group costs the launches one map costs.  The 64-position blocks of the definition are per map.
 *   - After a batched call chip_debug_vlad_stage reads the stages of the call's LAST map.  The single calls are batches of one.
 * Status, in this order: a NULL ctx / fmaps / v or n_maps < 0 CHIP_ERR_INVALID_ARG; positions or layout outside chip_vlad's limits
 * CHIP_ERR_UNSUPPORTED (both before the ctx is touched); a chip_create_multi or sharded ctx CHIP_ERR_UNSUPPORTED; no weights set
 * CHIP_ERR_BUSY; K*C against D / in_dim CHIP_ERR_UNSUPPORTED (the append); n_maps == 0 CHIP_OK (first_index is filled).          */
typedef struct chip_project_plan_out {
    int32_t width;             /* descriptors one shared pass serves                                          */
    int32_t slab;              /* elements of x per descriptor and slab                                       */
    int32_t lds_bytes;         /* dynamic LDS of a shared pass: 2 slabs x width descriptors x slab x 4 bytes  */
    int32_t single_lds_bytes;  /* dynamic LDS of a single launch: in_dim x 4 bytes                            */
    int32_t block;             /* threads per workgroup, both kernels                                         */
    int32_t reserved;
    int64_t passes;            /* reads of the matrix: shared_passes + single_launches                        */
    int64_t shared_passes;
    int64_t single_launches;
} chip_project_plan_out;
int chip_project_plan(int32_t in_dim, int32_t matrix_type, int64_t n, chip_project_plan_out *out);
int chip_debug_project_last(chip_ctx *ctx, int64_t passes[2], int64_t descriptors[2], int32_t *width);
int chip_vlad_batch(chip_ctx *ctx, const float *fmaps, int32_t n_maps, int32_t positions, int32_t layout, float *v /* n_maps x clusters*channels, host */);
int chip_db_append_vlad_batch_f32(chip_ctx *ctx, const float *fmaps, int32_t n_maps, int32_t positions, int32_t layout, uint32_t flags,
                                  int64_t *first_index);

/* ------------------------------------------------------------------------------------------ scan + top-k
 * Replaces  u = v.transpose() * M.leftCols(k); maxCoeff(); last-index argmax  (src/Cerebro.cpp:1026-1043)
 * generalised to top-K (the compiled-out faiss variants use K=5, src/Cerebro.cpp:460).
 * Scores are fp64 accumulations of exact fp32 products in the fixed order of DESIGN.md 3; ordering is
 * (score descending, index DESCENDING) so K=1 is the reference's "last index attaining the max".
 * Unused slots (k < K): score = -inf, idx = -1.  scores/idx are nq*topk, query-major.                   */
int chip_query_rows(chip_ctx *ctx, int64_t k, const int64_t *query_rows, int32_t nq, int32_t topk,
                    double *scores, int64_t *idx);
int chip_query_vectors_f32(chip_ctx *ctx, int64_t k, const float *queries, int32_t nq, int32_t topk,
                           double *scores, int64_t *idx);
/* double query vectors: as they are on a double-row DB; on a float-row DB they must be float32-representable (else
 * CHIP_ERR_NOT_F32 -- a rounded query would silently change scores). */
int chip_query_vectors_f64(chip_ctx *ctx, int64_t k, const double *queries, int32_t nq, int32_t topk,
                           double *scores, int64_t *idx);
/* The whole score vector  u = v^T * M.leftCols(k)  of ONE query row (src/Cerebro.cpp:1026; the reference's debug plot consumes
 * all of u, :1047-1052) -- same arithmetic, same bits as the scores chip_query_rows selects from.  u: k doubles (host).
 * A chip_create_multi ctx fills all of u.  A sharded ctx of the one-process-per-GPU layout fills only the entries of the rows THIS
 * rank owns (u[i], i % shard_count == shard_rank), with or without an exchange; with an exchange attached the call is collective
 * (the query row is broadcast from its owner), without one the query row must still be in this rank's ring. */
int chip_query_scores(chip_ctx *ctx, int64_t k, int64_t query_row, double *u);

/* Many-query batched mode: Q query descriptors (host, Q x D fp32) against rows [0,k) in ONE pass of
 * the DB as an fp32 GEMM on the matrix cores (v_mfma_f32_32x32x2_f32) with a fused exact top-k.  Semantics are those of
 * the reference's compiled-out faiss variants (IndexFlatIP on float descriptors, src/Cerebro.cpp:390,422,455-472):
 * score = fp32 inner product, here defined as ONE k-ordered fmaf chain (bit-reproducible; differs from the fp64 scores
 * of chip_query_* by fp32 round-off, ~1e-7).  Ordering (score desc, index desc); unused slots -inf / -1.
 * Requires D % 32 == 0 and float rows.  Worth it from Q ~ 40 upwards (arithmetic intensity Q/2 flop/B vs the 19.7 flop/B ridge).
 * Sharded DBs: a chip_create_multi ctx runs one pass per device over the rows it owns and merges the per-device lists on
 * devices[0]; a sharded ctx with an attached communicator does the same collectively (ncclAllGather of Q x topk entries per rank,
 * the same result on every rank); a sharded ctx WITHOUT an exchange answers for its own rows only (global indices) -- the host
 * merges.  Results are those of one device holding the whole DB, bit for bit (exact selection under a total order).
 * Outside the normal range the chain is IEEE fp32, step by step (tests/test_batch_edges_gpu.py): it overflows to +-inf where a
 * chained fmaf does (finite rows and queries never give NaN), subnormal inputs, products and partial sums are not flushed, and
 * the sign of a zero score is the chain's (-0.0 only where it ends in a negative underflow; +0.0 and -0.0 tie, index desc).
 * Queries are NOT validated: a NaN score (a NaN query element, 0 x inf, inf - inf) never enters a list, so such a query gets
 * fewer than topk entries (a NaN query: none); a real row scoring -inf precedes an unused slot (-inf, -1).                     */
int chip_query_batch_f32(chip_ctx *ctx, int64_t k, const float *queries, int32_t Q, int32_t topk,
                         float *scores /* Q x topk */, int64_t *idx /* Q x topk */);

/* The same mode on a DOUBLE-row DB, with the rows narrowed to float on their way into the GEMM.  The reference's DB is always
 * MatrixXd and its faiss variants index X.cast<float>() and search with the cast query (src/Cerebro.cpp:422,455,569,604,807,840):
 * every row element x enters as (float)x -- IEEE round to nearest even, what Eigen's cast<float>() and numpy's astype(float32) do --
 * and then the semantics of chip_query_batch_f32 apply unchanged (one k-ordered fmaf chain, (score desc, index desc)).  The cast is
 * lossy, and this library never rounds silently (CHIP_ERR_NOT_F32, CHIP_APPEND_ALLOW_ROUNDING): it is opt-in through THIS entry
 * point, and chip_query_batch_f32 keeps returning CHIP_ERR_UNSUPPORTED on double rows.  On a float-row ctx the two calls are the same
 * code path and return the same bits.  Arguments, limits (D % 32 == 0, topk, Q), CHIP_ERR_RANGE, group contexts and sharded contexts
 * with and without an exchange (collective behaviour, agreement round, failure mark) exactly as chip_query_batch_f32.
 * The cast is v_cvt_f32_f64, bit for bit numpy's astype(float32) over the whole double range (tests/test_batch_edges_gpu.py): beyond
 * the halfway point above FLT_MAX it gives +-inf (the scores then follow the IEEE rules above), into the subnormal range it rounds
 * to nearest even without flushing, a non-zero double below half the smallest subnormal gives a zero of its sign.  With topk > 8 a double-row DB is always scanned with the 128 x 128 tile (the DB is streamed once per 128 queries). */
int chip_query_batch_cast_f32(chip_ctx *ctx, int64_t k, const float *queries, int32_t Q, int32_t topk,
                              float *scores /* Q x topk */, int64_t *idx /* Q x topk */);

/* The same mode with a prefix PER QUERY, and with queries taken from DB rows (ABI 7, additive).  Bulk loop detection is causal: a node
 * restarted from its state, a replay, a second session searched against a first, the reference's faiss__naive_loopcandidate_generator
 * and faiss_clique_loopcandidate_generator (src/Cerebro.cpp:415-473, 558-650) all let query row i see rows [0, i - lag) only, and every
 * query already sits in the DB on the device.
 *   - chip_query_batch_rows_f32 (Cerebro.cpp:415-473): query j is DB row query_rows[j], gathered on the device, against rows [0, k[j]).
 *   - chip_query_batch_rows_cast_f32 (Cerebro.cpp:415-473): the same on a double-row DB; DB rows AND query rows enter as (float)x, round to
 *     nearest even (v_cvt_f32_f64 in both places).
 *   - chip_query_batch_prefix_f32 / chip_query_batch_prefix_cast_f32 (Cerebro.cpp:415-473): query j is the host vector queries + j * D,
 *     against rows [0, k[j]).
 * Definition: entry j of the result is, bit for bit, what chip_query_batch_f32(ctx, k[j], q_j, 1, topk, ..) returns, q_j being the caller's
 * vector or row query_rows[j] as floats (chip_query_batch_cast_f32 and (float)x on double rows).  Everything else is that mode's: one
 * k-ordered fp32 fmaf chain, (score desc, index desc), unused slots -inf / -1, a NaN score never enters a list.  k[j] may exceed
 * query_rows[j]: the row then meets itself.  Results come back in the caller's order.
 * How a call runs: the queries are stable-sorted by k and walked in groups of at most CHIP_QUERY_PREFIX_GROUP; a group is one gather launch
 * (or the upload and transpose of host vectors), one GEMM launch, one merge launch, one copy back and at most one host wait.  The GEMM
 * walks, per query tile, only the DB tiles below the largest prefix of that tile, and clips each query's scan at its own prefix: a causal
 * self-join costs about half the DB tiles of the rectangle.  A group picks the 256 x 256 or 128 x 128 tile as chip_query_batch_f32 does.
 * Status, all checked before anything is launched or written: a NULL pointer or Q < 1 CHIP_ERR_INVALID_ARG; D % 32 != 0, topk outside
 * [1, CHIP_MAX_TOPK], the _f32 entries on double rows, a chip_create_multi or sharded ctx CHIP_ERR_UNSUPPORTED (a query row of a sharded
 * DB lives on one rank only: prefix calls on group and sharded contexts are not part of this interface yet); k[j] < 0, k[j] > the
 * published length, or a query row outside [0, published length) CHIP_ERR_RANGE.
 *   - chip_query_prefix_plan (Cerebro.cpp:415-473; no ctx, no device): the order and the work of a call, from the functions the call sizes
 *     itself with.  elem: 4 float rows, 8 double rows.  order (Q entries, may be NULL): order[i] = the caller's position of the i-th
 *     query walked.  units and units_rect count tiles of the shape their group has; a call whose groups differ in shape (a partial last
 *     group on the 128 tile behind full groups on the 256 tile) sums tiles of two sizes, so units / units_rect is a measure of work
 *     only where tile_full == tile_last (or there is one group).  A NULL k / out or Q < 1 CHIP_ERR_INVALID_ARG; a negative k[j] CHIP_ERR_RANGE; elem or topk CHIP_ERR_UNSUPPORTED.
 *   - chip_debug_query_prefix_last (Cerebro.cpp:415-473): what the ctx's last prefix call did.  units_claimed is the sum, over groups and
 *     query tiles, of the work counters the kernel itself advanced (read back after each launch), so it is the kernel that is shown to
 *     skip the tiles; units_planned is the host's count, chip_query_prefix_plan's `units`.                                            */
#define CHIP_QUERY_PREFIX_GROUP 4096   /* queries per group */
typedef struct chip_query_prefix_plan_out {
    int32_t group_size;    /* CHIP_QUERY_PREFIX_GROUP                                                                     */
    int32_t groups;
    int32_t tile_full;     /* rows of the (square) tile of a full group: 256 or 128; 0 when the call has no full group    */
    int32_t tile_last;     /* of the last group                                                                           */
    int64_t qtiles;        /* query tiles, all groups                                                                     */
    int64_t units;         /* DB tiles walked: sum over query tiles of ceil(max k in the tile / tile rows)                */
    int64_t units_rect;    /* the same query tiles at ONE k = max over the call: what chip_query_batch_f32 would walk     */
} chip_query_prefix_plan_out;
typedef struct chip_query_prefix_last {
    int32_t groups, launches, waits, reserved;
    int64_t units_claimed, units_planned;
} chip_query_prefix_last;
int chip_build_has_query_prefix(void);   /* 1 */
int chip_query_batch_rows_f32(chip_ctx *ctx, const int64_t *query_rows, const int64_t *k, int32_t Q, int32_t topk,
                              float *scores /* Q x topk */, int64_t *idx /* Q x topk */);
int chip_query_batch_rows_cast_f32(chip_ctx *ctx, const int64_t *query_rows, const int64_t *k, int32_t Q, int32_t topk,
                                   float *scores /* Q x topk */, int64_t *idx /* Q x topk */);
int chip_query_batch_prefix_f32(chip_ctx *ctx, const int64_t *k, const float *queries, int32_t Q, int32_t topk,
                                float *scores /* Q x topk */, int64_t *idx /* Q x topk */);
int chip_query_batch_prefix_cast_f32(chip_ctx *ctx, const int64_t *k, const float *queries, int32_t Q, int32_t topk,
                                     float *scores /* Q x topk */, int64_t *idx /* Q x topk */);
int chip_query_prefix_plan(const int64_t *k, int32_t Q, int32_t elem, int32_t topk, int32_t *order /* Q, may be NULL */,
                           chip_query_prefix_plan_out *out);
int chip_debug_query_prefix_last(chip_ctx *ctx, chip_query_prefix_last *out);

/* ------------------------------------------------------------------------------------------ the tick
 * One pass of the while-loop body of Cerebro::descrip_N__dot__descrip_0_N (src/Cerebro.cpp:956-1100) for
 * l = wholeImageComputedList_size().  Defaults (chip_dot_params_default): LOCALITY_THRESH 12 (:912),
 * DOT_PROD_THRESH (double)(float)0.85 (:913,:1056), lag 50 (:914,:1019), >=3 new rows (:962), k > 5 (:1022). */
typedef struct {
    int32_t locality;
    int32_t lag;
    int32_t min_new;
    int32_t min_k;
    double  thresh;
} chip_dot_params;
void chip_dot_params_default(chip_dot_params *p);

enum { CHIP_TICK_SKIPPED = 0,   /* l - last_l < min_new: nothing done, last_l NOT advanced (:962-966)     */
       CHIP_TICK_TOO_SHORT = 1, /* ran, but k = l - lag <= min_k (:1022 else-branch); last_l = l          */
       CHIP_TICK_SCANNED = 2,   /* scan + decision executed; last_l = l                                   */
       CHIP_TICK_FAILED = 3 };  /* sharded ticks only, never returned with CHIP_OK: a shard could not take part; the collecting
                                   call returns CHIP_ERR_SHARD_FAILED on every rank and last_l is as before the tick -- unless a
                                   LATER tick had been enqueued by then (pipelined form): that tick's last_l = l stands      */

typedef struct {
    int32_t status;      /* CHIP_TICK_*                                                                   */
    int32_t found;       /* 1 iff the :1056 criterion fired -> foundLoops.push_back (:1078-1081)          */
    int64_t idx_curr;    /* l-1                (wholeImageComputedList index of t_curr)                   */
    int64_t idx_prev;    /* u_argmax           (index of t_prev)                                          */
    double  score;       /* u_max                                                                         */
    int64_t argmax[3];   /* u_argmax, um_argmax, umm_argmax                                               */
    double  maxv[3];     /* u_max, um_max, umm_max                                                        */
} chip_tick_result;

/* Synchronous tick (single-GPU ctx, shard_count == 1).
 * Environment, read at chip_create: CHIP_TICK_RESIDENT=1 turns ticks over prefixes of up to 512 MiB into commands to a scan kernel
 * that stays on the chip between ticks (no launch per tick: ~4.7 us less per call back to back, ~14 us at the reference's 10 Hz
 * cadence; same results).  The instance leaves by itself once NO tick has arrived for a whole lease (CHIP_RESIDENT_LEASE_MS,
 * default 250) -- so at 10 Hz it never leaves by itself.  The library itself pauses it around everything of its own that frees /
 * allocates device memory, grows the DB by a segment or wants the whole chip (no instance is launched until that section is over;
 * ticks that arrive meanwhile are launched).  Calls of OTHER libraries in the same process that wait for the whole device
 * (hipFree, hipMalloc of a new pool block, hipDeviceSynchronize) would wait for as long as ticks keep coming: bracket them with
 * chip_resident_pause / chip_resident_resume, or leave the mode off in such a process.  Off by default. */
int chip_loop_tick(chip_ctx *ctx, int64_t l, const chip_dot_params *p, chip_tick_result *out);
/* Retire the resident scan instance (waits until it has left the chip, <= one tick) and keep the mode from launching another one
 * until the matching chip_resident_resume; ticks in between are ordinary launches with identical results.  Calls nest.  CHIP_OK and
 * no effect on a ctx that does not run the mode.  Thread-safe against the tick, append and PnP threads (ABI 6). */
int chip_resident_pause(chip_ctx *ctx);
int chip_resident_resume(chip_ctx *ctx);
/* Pipelined form: enqueue up to CHIP_MAX_INFLIGHT - 1 ticks without host synchronisation, collect later.  Scans run
 * back to back on an internal stream; the one-workgroup merge of tick i (ctx stream) overlaps the scan of tick i+1.
 *
 * Ticks that share a DB pass.  Queued ticks do not depend on one another (status and last_l are settled at enqueue, the queries
 * are published rows), so on a plain single-GPU ctx with float or double rows, on its own streams, an enqueue over a LONG prefix (beyond
 * CHIP_SCAN_OVERLAP_GIB, 8 GiB) that finds a scan of the ctx still running PARKS its tick instead of launching it; parked ticks
 * leave together as ONE pass over [0, max k) with 3 T queries (T <= CHIP_TICK_COALESCE, default 5; 0 = off), every tick seeing
 * only its own prefix [0, k_t).  Which rows: whole 4 KiB batches -- float rows with D % 1024 == 0 whose 3 T queries fit the LDS (D = 4096:
 * T <= 3), double rows with D % 512 == 0 up to D = 4608, T = 2 (the queries that do not fit the LDS are read in place, out of the L2);
 * chip_debug_multi_plan says what a given shape gets.  FOUR ticks (float rows up to D = 4096, chip_debug_prefilter_plan) leave as a pass
 * that scores in fp32 and then proves, per query, which rows can be in the exact top-8 and scores those in fp64 in the usual order:
 * same records; a tick whose proof does not go through (scores closer together than the fp32 error bound taken from
 * chip_info.row_norm_max) runs again alone at its collect.  FIVE ticks (the same shapes, chip_debug_halfq_plan) leave as a pass of the
 * same kind whose 15 queries are staged in LDS as fp16, scaled by a power of two taken from row_norm_max: same proof with a larger error
 * bound, same records; the pass parked behind a tick that was launched alone takes four, five only behind a shared pass.  CHIP_TICK_COALESCE=2 / 3 / 4 are what they were (4: passes of four through the fp32 pass, never the fp16-query one).  Every other ctx launches its ticks one by one.  Results, status codes, CHIP_ERR_BUSY, last_l, chip_loop_reset, skipped / too-short ticks in
 * between, appends between enqueue and collect and out-of-order collects are exactly those of ticks launched one by one.  A tick
 * that arrives while no scan is running is launched at once, alone; chip_loop_tick, short prefixes and caller-supplied streams
 * (chip_set_stream) never park.  Nothing stays parked while its caller cannot release it.  Parked ticks are submitted by:
 *   chip_loop_tick_enqueue of the T-th tick, or of any tick that does not park;   chip_loop_tick_collect of a parked slot, and a
 *   collect that is about to block on the newest pass submitted;   chip_loop_tick;   chip_query_rows / _vectors_* / _scores;
 *   chip_scan_local, chip_merge_decide[_enqueue];   chip_loop_ticks_bulk;   chip_synchronize, chip_destroy, chip_set_stream / chip_reset_stream,
 *   chip_resident_pause, chip_profile_enable / _reset / _scan.
 * A HIP failure while a pass is submitted is returned by the collect of each tick it concerned.  With profiling on a pass is one
 * launch: one event pair, bytes_per_launch_last = the bytes of that pass. */
#define CHIP_MAX_INFLIGHT 64
int chip_loop_tick_enqueue(chip_ctx *ctx, int64_t l, const chip_dot_params *p, int32_t slot);
int chip_loop_tick_collect(chip_ctx *ctx, int32_t slot, chip_tick_result *out);
int64_t chip_loop_last_l(const chip_ctx *ctx);
void chip_loop_reset(chip_ctx *ctx);
int chip_build_has_tick_coalesce(void);   /* 1: this build can serve several pipelined ticks with one pass (ABI 7, additive) */
/* Test aids.  _stats: passes that served more than one tick and the ticks they served.  _force: while on, a tick that may share a
 * pass parks even when no scan is running (the release rules above are unchanged; switching it off releases).  _decide: the parking
 * policy alone, no ctx: 0 launch now, 1 park, 2 park and release all, for n_parked ticks waiting, t_max per pass, a scan running or not. */
int chip_debug_coalesce_stats(chip_ctx *ctx, int64_t *passes, int64_t *ticks);
int chip_debug_coalesce_force(chip_ctx *ctx, int32_t on);
int chip_debug_coalesce_decide(int32_t n_parked, int32_t t_max, int32_t scan_running);

/* Bulk ticks (ABI 7, additive): the records of a whole SEQUENCE of ticks from many-query passes -- for a node restarted from its state, a
 * replay, a second session searched against a first (Cerebro.cpp:956-1100 run over rows that are all there already).
 * Definition: out[t] is, bit for bit in every field, the record the t-th call of
 *     chip_loop_tick(ctx, l[0], p, ..), chip_loop_tick(ctx, l[1], p, ..), ...
 * returns on the same DB, starting from a loop state whose last_l is the argument; *last_l_out the loop state after the last one.  SKIPPED
 * and TOO_SHORT ticks and the advance of last_l follow the rule of the tick itself (one function serves both).  scores / idx of a SCANNED
 * tick are what chip_query_rows(ctx, l - lag, {l-1, l-2, l-3}, 3, topk, ..) returns: fp64 scores in the order of DESIGN.md 3, (score
 * desc, index desc), unused slots -inf / -1; of every other tick -inf / -1.
 * How a call runs: the scanned ticks are stable-sorted by k and walked in groups of at most CHIP_BULK_TICKS_GROUP ticks (three queries
 * each, so a tick never straddles a CHIP_QUERY_PREFIX_GROUP).  A group is the gather, the prefixed GEMM and the list merge of
 * chip_query_batch_rows_f32 with a list length of the library's own, then ONE launch that, per tick, proves from the fp32 lists which
 * rows can be in each exact top-topk (the certificate of DESIGN.md 3: the GEMM's score is one fp32 chain of D terms, inside the same bound E),
 * scores those rows in fp64 in the scan's own order, ranks them and applies the accept rule; one copy back, one host wait.  A tick whose
 * proof does not go through runs again alone through the exact scan after the last group, so the answer never depends on the data.  Where
 * the row-norm bound is out of the fp32 range (row_norm_max^2 > 2^120) every scanned tick takes the exact path.
 * State: a pure function of the DB and its arguments.  The ctx's own last_l, slots and parked ticks are neither read nor written (parked
 * ticks are released first, as by the calls listed above); the query lock is held and the resident scan paused for the call.
 * Status, all checked before anything is launched or written: NULL ctx / l / out or T < 1 CHIP_ERR_INVALID_ARG; topk outside [1, 8],
 * D % 32 != 0, double rows, a chip_create_multi or sharded ctx CHIP_ERR_UNSUPPORTED (double rows would need the rounding of the cast folded
 * into E: deliberately not part of this interface); an l[t] for which the sequential call would return CHIP_ERR_RANGE: CHIP_ERR_RANGE.
 * One refusal more than the tick has: a scanned tick whose prefix k = l - lag is negative or beyond the published length (only with a
 * negative lag, or min_k below -lag) is CHIP_ERR_RANGE here and in chip_bulk_ticks_plan; chip_loop_tick does not check it.
 *   - chip_bulk_ticks_plan (no ctx, no device): status and k of every tick (k[t] = 0 where the tick is not scanned), the final last_l and
 *     the grouping, from the functions the call itself uses.  units / units_rect count DB tiles as chip_query_prefix_plan does.
 *   - chip_debug_bulk_ticks_last: what the ctx's last bulk call did.  launches counts the group launches (four per group) and not those
 *     of the exact reruns; certified / uncertified are ticks; rescored_rows the rows scored exactly by the finishing launches.            */
#define CHIP_BULK_TICKS_GROUP 1365   /* ticks per group: 4095 queries */
#define CHIP_BULK_TICKS_MAX_TOPK 8
typedef struct chip_bulk_ticks_plan_out {
    int32_t group_ticks;   /* CHIP_BULK_TICKS_GROUP                                                                       */
    int32_t groups;
    int32_t tile_full;     /* rows of the tile of a full group (256); 0 when the call has no full group                   */
    int32_t tile_last;     /* of the last group: 256 or 128; 0 when no tick is scanned                                    */
    int64_t ticks_scanned, ticks_skipped, ticks_too_short;
    int64_t units, units_rect;
    int64_t last_l;        /* the loop state after the last tick                                                          */
} chip_bulk_ticks_plan_out;
typedef struct chip_bulk_ticks_last {
    int32_t groups, launches, waits;
    int32_t list_len;      /* KL: entries per fp32 list                                                                   */
    int64_t certified, uncertified, rescored_rows, exact_reruns;
    double E;              /* the error bound the certificates used (0 where every tick took the exact path)              */
} chip_bulk_ticks_last;
int chip_build_has_bulk_ticks(void);   /* 1 */
int chip_loop_ticks_bulk(chip_ctx *ctx, const int64_t *l, int32_t T, const chip_dot_params *p /* NULL: defaults */,
                         int64_t last_l, int32_t topk /* 1 .. 8 */,
                         chip_tick_result *out /* T */, double *scores /* T x 3 x topk, may be NULL */,
                         int64_t *idx /* T x 3 x topk, may be NULL */, int64_t *last_l_out /* may be NULL */);
int chip_bulk_ticks_plan(const int64_t *l, int32_t T, const chip_dot_params *p /* NULL: defaults */, int64_t last_l, int64_t n_rows,
                         int32_t *status /* T */, int64_t *k /* T */, chip_bulk_ticks_plan_out *out);
int chip_debug_bulk_ticks_last(chip_ctx *ctx, chip_bulk_ticks_last *out);

/* Test aids (ABI 7, additive): WHICH kernel a top-k scan ran.  The scan dispatcher chooses between four kernel families and their
 * template instantiations from the prefix size, the row size, the query count, the kind of call and the CHIP_SCAN_* knobs; all of
 * them compute the same bits, and tests/test_scan_forms_gpu.py holds every one of them to that.  The record is filled where the
 * instantiation is chosen, host side only: no kernel argument, nothing on the device depends on it.  Fields a family does not have are 0.
 *   chip_debug_last_scan  the last top-k scan launch of this ctx (family 0 before the first one); `launches` counts them.
 *   chip_debug_scan_plan  the same record WITHOUT a device or a ctx: what a plain single-GPU ctx of n_cus compute units, created
 *                         under the CHIP_SCAN_* / CHIP_TICK_* variables of the environment as it is now, on its own streams and with
 *                         profiling off, launches for nq queries (K list entries each) over n_rows rows of D elements of elem
 *                         bytes -- computed by the functions the enqueue path itself runs.  Returns what that launch would
 *                         return (CHIP_OK, CHIP_ERR_UNSUPPORTED, ...); `launches` stays 0. */
#define CHIP_SCAN_FAMILY_NONE    0
#define CHIP_SCAN_FAMILY_ONE_ROW 1   /* db_scan_topk<T, NQ, U, FULL, NT, 1>: one row per wave at a time                          */
#define CHIP_SCAN_FAMILY_WIDE    2   /* db_scan_topk_wide<NQ, NG, FULL>: double rows, NG of the NQ queries read in place           */
#define CHIP_SCAN_FAMILY_ROWS    3   /* db_scan_topk_rows<T, NQ, R, NTL>: R rows per wave in flight; carries the fused tick        */
#define CHIP_SCAN_FAMILY_MULTI   4   /* db_scan_topk_multi<T> / db_scan_shared_f64<T, NG>: `ticks` pipelined ticks share one pass     */
#define CHIP_SCAN_FAMILY_PREFILTER 5 /* db_scan_prefilter<NG>: four pipelined ticks share one fp32 pass; tick_rescore scores the proven candidates exactly */
#define CHIP_SCAN_FAMILY_HALFQ   6   /* db_scan_halfq: five pipelined ticks share one fp32 pass over queries staged as fp16; tick_rescore as above */
#define CHIP_SCAN_CALL_QUERY      0  /* chip_query_rows / chip_query_vectors_*: lists out                                         */
#define CHIP_SCAN_CALL_TICK       1  /* chip_loop_tick_enqueue: a pipelined tick                                                   */
#define CHIP_SCAN_CALL_TICK_SYNC  2  /* chip_loop_tick: the synchronous tick                                                       */
typedef struct {
    int32_t family;        /* CHIP_SCAN_FAMILY_*                                                                                   */
    int32_t elem;          /* storage element size: 4 float rows, 8 double rows                                                    */
    int32_t nq, K;         /* queries of the launch (multi: 3 per tick) and list entries kept per query (a fused tick keeps 1)     */
    int32_t U, NT, FULL;   /* one-row: 16-byte loads per lane and batch, load path (1 builtin, 6 asm-issued, 8 asm-issued with fp64-staged
                              queries), rows of whole batches;  wide / multi: FULL / U alone                                       */
    int32_t NG;            /* wide / multi (double rows): queries read in place                                                    */
    int32_t R, NTL;        /* rows / multi: rows per wave and pass;  rows: 1 non-temporal loads                                    */
    int32_t ticks;         /* multi: ticks served by the pass                                                                      */
    int32_t q64;           /* queries staged in LDS as fp64 (multi, double rows: how many of the nq)                               */
    int32_t claimed;       /* rows: the waves of a workgroup claim their rows from a counter instead of the static map            */
    int32_t fused;         /* rows: the launch writes the tick's decision record itself, no merge kernel follows                   */
    int32_t grid, block;   /* workgroups, threads per workgroup                                                                    */
    int32_t wg_per_cu;     /* workgroups of that shape a compute unit is meant to hold (their LDS must fit 160 KiB together)       */
    int32_t lds_bytes;     /* dynamic LDS per workgroup                                                                            */
    int64_t n_rows;        /* local rows the launch reads                                                                          */
    int64_t launches;      /* top-k scan launches of the ctx so far, this one included                                             */
} chip_debug_scan_launch;
int chip_debug_last_scan(chip_ctx *ctx, chip_debug_scan_launch *out);
int chip_debug_scan_plan(int32_t D, int32_t elem, int32_t nq, int32_t K, int64_t n_rows, int32_t call, int32_t n_cus,
                         chip_debug_scan_launch *out);
/* The shared pass of n_ticks pipelined ticks (family CHIP_SCAN_FAMILY_MULTI) without a device or a ctx, from the function the launch
 * sizes itself with: nq = 3 n_ticks, ticks, R, q64 = queries staged in LDS as fp64 (double rows; float rows stage all of theirs as fp32),
 * NG = queries read in place, lds_bytes (queries + the waves' lists of K entries), grid (one workgroup per compute unit) and block.
 * CHIP_ERR_UNSUPPORTED where a plain single-GPU ctx of that shape has no such pass and launches its ticks one by one (ABI 7, additive). */
int chip_debug_multi_plan(int32_t D, int32_t elem, int32_t n_ticks, int32_t K, int32_t n_cus, chip_debug_scan_launch *out);
/* The prefilter pass of four pipelined ticks (family CHIP_SCAN_FAMILY_PREFILTER, float rows) the same way: nq = 12, ticks = 4, NG = queries read
 * in place (the others are staged in LDS as fp32), lds_bytes, grid, block.  CHIP_ERR_UNSUPPORTED where a ctx of that shape has no such pass and
 * releases at most three ticks together (ABI 7, additive). */
int chip_debug_prefilter_plan(int32_t D, int32_t elem, int32_t K, int32_t n_cus, chip_debug_scan_launch *out);
/* The five-tick pass (family CHIP_SCAN_FAMILY_HALFQ, float rows) the same way: nq = 15, ticks = 5, NG = 0 (every query staged in LDS as fp16),
 * lds_bytes, grid, block.  CHIP_ERR_UNSUPPORTED where a ctx of that shape has no such pass and releases at most four ticks together (additive). */
int chip_debug_halfq_plan(int32_t D, int32_t elem, int32_t K, int32_t n_cus, chip_debug_scan_launch *out);
/* The scale and the error bound such a pass over rows of norm at most row_norm_max is launched with: the staged queries are fl16(2^e q), and
 * |score of the pass - exact score| <= E for every pair of published rows.  No device needed (additive). */
int chip_debug_halfq_bound(int32_t D, double row_norm_max, int32_t *e, double *E);
/* Prefilter passes of either kind (four ticks, five ticks) submitted, the ticks they served, and those of them whose certificate did not hold (counted at collect: such a tick was run
 * again alone, and its caller got that record). */
int chip_debug_prefilter_stats(chip_ctx *ctx, int64_t *passes, int64_t *ticks, int64_t *uncertified);

/* Sharded tick, three phases (host does the exchange between 1 and 2):
 *  1. chip_scan_local: scan this rank's share of rows [0,k), k = l - lag, for the three queries l-1,l-2,l-3 and
 *     leave its 3 x topk list (chip_topk_entry, global indices) in DEVICE memory at dev_out (caller-owned,
 *     3*topk*sizeof(chip_topk_entry) bytes).  *status gets CHIP_TICK_*; when it is not CHIP_TICK_SCANNED nothing was
 *     enqueued and phases 2-3 are skipped by every rank alike.
 *     Stream semantics: the list is written by a small merge kernel on the ctx stream (chip_set_stream), so work
 *     enqueued there afterwards (the all-gather) sees it and dev_out / gathered buffers may be reused every tick.
 *     The scan itself runs on an internal stream: the next tick's scan overlaps this tick's merge + all-gather.
 *  2. host: all-gather dev_out of every rank -> gathered[G][3][topk] (on the ctx stream).
 *  3. chip_merge_decide (synchronous) or chip_merge_decide_enqueue + chip_loop_tick_collect (pipelined):
 *     merge the G lists per query, apply the :1056 criterion, return the result.                          */
typedef struct { double score; int64_t idx; } chip_topk_entry;
int chip_scan_local(chip_ctx *ctx, int64_t l, const chip_dot_params *p, int32_t topk, void *dev_out, int32_t *status);
int chip_merge_decide(chip_ctx *ctx, int64_t l, const chip_dot_params *p, const void *dev_gathered, int32_t n_lists,
                      int32_t topk, chip_tick_result *out);
int chip_merge_decide_enqueue(chip_ctx *ctx, int64_t l, const chip_dot_params *p, const void *dev_gathered, int32_t n_lists,
                              int32_t topk, int32_t slot);
/* Test aid (ABI 7, additive): the list merge alone, on lists the caller writes.  Every scan result leaves through one of two kernels;
 * this call copies `lists` (host, [n_lists][nq][K]: each list sorted by (score descending, index descending), indices unique per query,
 * no NaN, unused slots (-inf, -1), a failed shard's list (-inf, -2) in every entry) to device memory, launches
 *   form 0: topk_merge<nq>, nq = 1 .. CHIP_MAX_NQ, through the launch helper of the tick, the query and the exchange paths; with `result`
 *           non-NULL the kernel also writes the decision record of tick l under p (as chip_merge_decide does; p must be given then);
 *   form 1: topk_merge_batch, the merge of the many-query mode, nq a multiple of 4: one workgroup per four queries, list stride nq;
 *           no record (result must be NULL),
 * waits, and copies the merged [nq][K] lists to `out` (host) as the kernel wrote them: a failed list's mark is out[0].idx == -2 (form 1:
 * in the first entry of each workgroup's four queries).
 * tests/test_merge_gpu.py runs tests/merge_cases.py through it.  Synchronous, takes the query lock.  CHIP_ERR_UNSUPPORTED: group ctx,
 * K outside 1 .. CHIP_MAX_TOPK, n_lists > 512, an nq or a form that does not exist; CHIP_ERR_INVALID_ARG: NULL pointers, n_lists < 1. */
int chip_debug_merge_lists(chip_ctx *ctx, int32_t form, const chip_topk_entry *lists, int32_t n_lists, int32_t nq, int32_t K,
                           chip_topk_entry *out, int64_t l, const chip_dot_params *p, chip_tick_result *result);
/* Test aid (ABI 7, additive): what the ctx's last prefilter pass (CHIP_SCAN_FAMILY_PREFILTER, four ticks, or _HALFQ, five) left in device
 * memory, so that tests/test_pass_lists_gpu.py and tests/test_rescore_gpu.py can hold the pass's own scores, lists and certificates to the
 * oracle's mirrors and not only the records that come out behind them.  It launches nothing and submits nothing (parked ticks stay parked):
 * it waits for the ctx's own streams, then copies.
 *   info   family, ticks T, grid (workgroups = lists per tick and query), wpb (waves per workgroup: workgroup b owns the rows r with
 *          r mod (grid wpb) in [b wpb, (b + 1) wpb)), K, the prefixes k[t], the error bound E handed to tick_rescore and, for _HALFQ, the
 *          exponent e of the queries' scale (0 otherwise);
 *   cand   [T][grid][3][K]: the pass's lists, (pass score widened to double, row), sorted by (score descending, index descending), unused
 *          entries (-inf, -1);
 *   exact  [T][3][K]: the lists tick_rescore wrote, exact scores of the candidates it kept;
 *   cert   [T][3]: 1 the query's certificate holds, 2 it does not.
 * Any output pointer may be NULL.  The list buffer is not reused before 64 further scans are enqueued and a tick that runs again alone takes
 * another buffer, so the copy is valid after the collects of the pass's window.  CHIP_ERR_BUSY before the first such pass,
 * CHIP_ERR_INVALID_ARG for a NULL or chip_create_multi ctx.  Synchronous, takes the query lock. */
typedef struct {
    int32_t family, ticks, grid, wpb, K;
    int32_t e;
    int64_t k[5];
    double E;
} chip_debug_pass_info;
int chip_debug_last_pass(chip_ctx *ctx, chip_debug_pass_info *info, chip_topk_entry *cand, chip_topk_entry *exact, uint32_t *cert);

/* ------------------------------------------------------------------------------------------ PnP-RANSAC
 * Replaces the body of StaticTheiaPoseCompute::PNP (src/DlsPnpWithRansac.cpp:192-240): theia::Ransac over
 * the DlsPnpWithRansac estimator (src/DlsPnpWithRansac.h:42-100).
 *   X  : N x 3 row-major, 3-D points in frame a            (w_X,  DlsPnpWithRansac.cpp:196)
 *   uv : N x 2 row-major, normalized image coords in b     (c_uv_normalized, :197)
 *   T  : 4x4 COLUMN-major b_T_a (Eigen Matrix4d layout)    (c_T_w = best_rel_pose.b_T_a, :239)
 * Returns CHIP_ERR_TOO_FEW_POINTS for N < 20 (:136-139; the reference returns confidence -1).  When no
 * hypothesis yields a model, status is CHIP_OK, *confidence = 0 and T is filled with NaN (the reference
 * returns an UNINITIALISED Matrix4d, :204; its caller only NaN-checks, Cerebro.cpp:1678).
 * n_hypotheses == 0: reference-faithful adaptive loop (<= max_iterations, early termination as
 * theia::Ransac; hypotheses are generated in parallel and the sequential rule is replayed on the host).
 * n_hypotheses  > 0: benchmark mode, exactly that many hypotheses, all scored, argmin cost with the lowest
 * hypothesis index winning ties (BASELINE config 3 uses 1000).                                         */
typedef struct {
    double  error_thresh;        /* 0.03   DlsPnpWithRansac.cpp:208 */
    double  min_inlier_ratio;    /* 0.7    :209 */
    int32_t max_iterations;      /* 50     :210 */
    int32_t min_iterations;      /* 5      :211 */
    int32_t use_mle;             /* 1      :212 */
    int32_t sample_size;         /* 15     DlsPnpWithRansac.h:45; 3 .. 16 and <= N accepted (else CHIP_ERR_UNSUPPORTED), each value
                                    held to the oracle hypothesis by hypothesis for PnP and ICP */
    double  failure_probability; /* 0.01   theia::RansacParameters default */
    uint64_t seed;               /* counter-based sampler seed (Theia's is time-seeded => nondeterministic) */
    int32_t n_hypotheses;        /* 0 = adaptive reference mode */
    int32_t sampler;             /* CHIP_SAMPLER_*: which permutation the 15 / 10 sample indices of a hypothesis are drawn from (ABI 5) */
} chip_ransac_params;
/* CHIP_SAMPLER_FRESH (default): a fresh identity permutation per hypothesis -- hypotheses are independent and are generated on the
 * device.  CHIP_SAMPLER_THEIA_PERSISTENT: theia::RandomSampler as written -- the permutation is initialised ONCE per estimation and
 * every hypothesis continues on the array the previous one left (one theia::Ransac, hence one sampler, per PNP / P3P_ICP call:
 * src/DlsPnpWithRansac.cpp:216-221, :95-100); the host sequences the swaps (S per hypothesis) and hands the kernels a sample table.
 * Both modes use the same counter-based draws (Theia's own generator is time-seeded, i.e. not reproducible).                     */
enum { CHIP_SAMPLER_FRESH = 0, CHIP_SAMPLER_THEIA_PERSISTENT = 1 };
void chip_ransac_params_default(chip_ransac_params *p);

typedef struct {
    int32_t n_iterations;     /* summary.num_iterations (:229)                                   */
    int32_t n_inliers;
    int32_t best_hypothesis;  /* index of the winning hypothesis, -1 if none                      */
    int32_t n_models;         /* hypotheses for which DlsPnp returned exactly one solution        */
    double  best_cost;
} chip_ransac_summary;

int chip_pnp_ransac(chip_ctx *ctx, const double *X, const double *uv, int32_t N, const chip_ransac_params *p,
                    double T_colmajor[16], float *confidence, uint8_t *inlier_mask /* N bytes, may be NULL */,
                    chip_ransac_summary *summary /* may be NULL */);

/* P independent estimations in one pair of launches -- e.g. the two role-swapped PNP calls the loop-candidate consumer
 * makes per image pair (src/Cerebro.cpp:1518 and :1572).  One wave per hypothesis is latency-bound at H = 1000, so
 * co-scheduled problems cost little more than one.  All problems share *p; problem i draws from seeds[i] (NULL: p->seed
 * for every problem) and its outputs (T_colmajor + 16 i, confidence[i], inlier_mask[i] (N[i] bytes; the array or any
 * entry may be NULL), summary[i]) are bit-identical to chip_pnp_ransac(X[i], uv[i], N[i]) with that seed.
 * Any N[i] < 20 fails the whole call with CHIP_ERR_TOO_FEW_POINTS before anything runs.                         */
int chip_pnp_ransac_batch(chip_ctx *ctx, int32_t P, const double *const *X, const double *const *uv, const int32_t *N,
                          const chip_ransac_params *p, const uint64_t *seeds, double *T_colmajor /* P x 16 */,
                          float *confidence /* P */, uint8_t *const *inlier_mask, chip_ransac_summary *summary /* P or NULL */);

/* ------------------------------------------------------------------------------------------ Umeyama-ICP-RANSAC
 * Replaces the RANSAC branch of StaticTheiaPoseCompute::P3P_ICP (src/DlsPnpWithRansac.cpp:65-121): theia::Ransac over
 * AlignPointCloudsUmeyamaWithRansac (src/DlsPnpWithRansac.h:104-166): 10-point sample -> AlignPointCloudsUmeyama ->
 * accept iff min(s, 1/s) > 0.9 (:137) -> b_T_a = [R t] -> L2 error (:152-164), threshold 0.1, MLE score.
 *   A, B : N x 3 row-major, the same 3-D points expressed in frames a and b (uv_X, uvd_Y, :15-16)
 * Status / T / confidence / mask / summary conventions are those of chip_pnp_ransac (N < 20 -> CHIP_ERR_TOO_FEW_POINTS,
 * :19-22).  chip_icp_params_default = chip_ransac_params_default with error_thresh 0.1 (:89) and sample_size 10 (.h:118). */
void chip_icp_params_default(chip_ransac_params *p);
int chip_icp_ransac(chip_ctx *ctx, const double *A, const double *B, int32_t N, const chip_ransac_params *p,
                    double T_colmajor[16], float *confidence, uint8_t *inlier_mask /* N bytes, may be NULL */,
                    chip_ransac_summary *summary /* may be NULL */);
/* The same estimation in two halves, so that it can run underneath something else -- the loop-candidate consumer computes
 * PNP(a->b), PNP(b->a) and P3P_ICP for one image pair (src/Cerebro.cpp:1518,1572,1629), and the ICP kernel is tiny:
 *   chip_icp_ransac_enqueue : copies A, B (the call returns once they are staged) and launches on the ctx's ICP stream;
 *   chip_icp_ransac_collect : waits for it and delivers exactly what chip_icp_ransac would have returned.
 * One estimation may be pending per ctx, single or batch (chip_icp_ransac_matched_batch_enqueue below): any ICP enqueue or
 * blocking ICP call while one is pending, a collect without an enqueue, and chip_icp_ransac_collect on a pending batch return
 * CHIP_ERR_BUSY.                                                                                                          */
int chip_icp_ransac_enqueue(chip_ctx *ctx, const double *A, const double *B, int32_t N, const chip_ransac_params *p);
int chip_icp_ransac_collect(chip_ctx *ctx, double T_colmajor[16], float *confidence, uint8_t *inlier_mask /* may be NULL */,
                            chip_ransac_summary *summary /* may be NULL */);

/* P independent estimations in ONE pair of launches (ABI 7, additive): the twin of chip_pnp_ransac_batch.  icp_models_batch runs on a
 * grid of ceil(H / 64) x P, icp_score_batch on H x P; what differs per problem (A, B, N, the seed, the sampler's multipliers) comes
 * from a table the ctx owns, copied to device memory in-stream and read through uniform loads (P = 1 launches the single pair).  All problems share *p; problem i draws from seeds[i] (NULL: p->seed for every problem)
 * and its outputs (T_colmajor + 16 i, confidence[i], inlier_mask[i] (N[i] bytes; the array or any entry may be NULL), summary[i])
 * are bit-identical to chip_icp_ransac(A[i], B[i], N[i]) with that seed, whatever P and whoever its neighbours are.  chip_icp_ransac
 * is this call with P = 1.  Any N[i] < 20 fails the whole call with CHIP_ERR_TOO_FEW_POINTS before anything runs; P < 1 or a NULL
 * pointer: CHIP_ERR_INVALID_ARG; P > CHIP_ICP_MAX_BATCH: CHIP_ERR_UNSUPPORTED.  Group ctxs: devices[0].                          */
#define CHIP_ICP_MAX_BATCH 16              /* = CHIP_MATCH_MAX_BATCH */
int chip_build_has_icp_batch(void);        /* 1 */
int chip_icp_ransac_batch(chip_ctx *ctx, int32_t P, const double *const *A, const double *const *B, const int32_t *N,
                          const chip_ransac_params *p, const uint64_t *seeds, double *T_colmajor /* P x 16 */,
                          float *confidence /* P */, uint8_t *const *inlier_mask, chip_ransac_summary *summary /* P or NULL */);

/* Test aids (ABI 7, additive): the record of EVERY hypothesis of the most recent estimation of a ctx, not only of its winner.
 * Both kernel pairs leave valid / cost / inlier count / pose / inlier mask per hypothesis (and the selection rule is replayed over
 * them on the host); these calls copy that out.  They read what a finished call left behind: they take the estimation's lock, wait
 * for the leg's stream, change nothing and launch nothing.  tests/test_ransac_hypotheses_gpu.py holds every row to the oracle.
 *   chip_debug_ransac_record  leg CHIP_RANSAC_LEG_PNP: problem `problem` of the last LAUNCH of chip_pnp_ransac / _batch / _matched
 *                             (a batch of more than 8 problems runs as several launches of up to 8; the record is that of the last
 *                             launch, its problems numbered from 0); leg CHIP_RANSAC_LEG_ICP: the last collected chip_icp_ransac /
 *                             _collect / _matched (problem 0 of 1) or problem `problem` of the last collected chip_icp_ransac_batch /
 *                             _matched_batch (of a matched batch: the problems that RAN, numbered from 0).  *shape first (it sizes the arrays), then any of
 *                               valid[H], cost[H], nin[H], T[H][16] column-major, mask[H][words] (bit i & 63 of word i >> 6 = point i),
 *                               PnP only: nsol[H] (cheirality-valid solutions; -1 singular system, -2 eigenvalue iteration gave up),
 *                                         sample[H][S] (the sampler's indices as pnp_build_solve used them).
 *                             Every output may be NULL.  The content is defined everywhere: a rejected hypothesis (valid 0) has cost
 *                             +inf, nin 0, T = NaN and an all-zero mask row -- the kernels do not write T or the mask of such a
 *                             hypothesis, nor the mask words beyond a problem's own ceil(N / 64) in a batch whose rows have the
 *                             stride of its widest problem; the copy is filled here, on the host.  In the adaptive mode
 *                             (n_hypotheses == 0) H is the initial iteration count: the rows after summary.n_iterations are there too.
 *   chip_debug_pnp_stage      what pnp_build_solve handed to pnp_eig_score in that launch, copied from device memory:
 *                             ok[H] (0: singular elimination), Tg[H][27] (t = Tg * vec(R)), Sg[H][27][27] (the action matrix; NaN
 *                             where ok is 0).  The rare loop form of the back-substitution in pnp_eig_score uses a hypothesis's Sg
 *                             slot as scratch, so Sg is what pnp_build_solve wrote only for launches made while
 *   chip_debug_pnp_keep_stage is on: the launch then copies Sg aside between the two kernels (device to device, off by default).
 * CHIP_ERR_BUSY: no finished estimation on that leg (none yet, the last one failed, or an ICP enqueue awaits its collect);
 * CHIP_ERR_INVALID_ARG: unknown leg, problem outside the launch, nsol / sample asked of the ICP leg.  Group ctxs: devices[0].      */
#define CHIP_RANSAC_LEG_PNP 0
#define CHIP_RANSAC_LEG_ICP 1
typedef struct {
    int32_t P;       /* problems of the launch                                             */
    int32_t H;       /* hypotheses per problem                                             */
    int32_t N;       /* correspondences of this problem                                    */
    int32_t words;   /* mask words per row: ceil(N / 64) of the launch's widest problem    */
    int32_t S;       /* sample size                                                        */
    int32_t sampler; /* CHIP_SAMPLER_*                                                     */
} chip_debug_ransac_shape;
int chip_debug_ransac_record(chip_ctx *ctx, int32_t leg, int32_t problem, chip_debug_ransac_shape *shape, int32_t *valid, double *cost,
                             int32_t *nin, double *T_colmajor, uint64_t *mask, int32_t *nsol, int32_t *sample);
int chip_debug_pnp_stage(chip_ctx *ctx, int32_t problem, int32_t *ok, double *Tg, double *Sg);
int chip_debug_pnp_keep_stage(chip_ctx *ctx, int32_t on);


/* ------------------------------------------------------------------------------------------ candidate verification front end
 * Replaces what the loop-candidate consumer runs per candidate BETWEEN the descriptor scan and the three pose solves:
 *   BFMatcher(NORM_HAMMING).match(d1, d2) over ORB descriptors          src/utils/PointFeatureMatching.cpp:38-41
 *   gms_matcher(kp1, size1, kp2, size2, matches).GetInlierMask(.., false, false)   :50-52, src/utils/GMSMatcher/gms_matcher.{h,cpp}
 *   the "< 150 matches" reject and pf_matches                           src/Cerebro.cpp:1487,1505
 *   make_3d_2d_collection__using__pfmatches_and_disparity (a->b, b->a)  PointFeatureMatching.cpp:95-154, Cerebro.cpp:1512,1566
 *   make_3d_3d_collection__using__pfmatches_and_disparity               PointFeatureMatching.cpp:159-195, Cerebro.cpp:1624
 * Rectification stays with the caller (OpenCV); detection is chip_orb_detect, description chip_orb_detect_describe, and the depth
 * images are chip_frame_put_disparity / chip_frame_put_stereo, all below.  Everything here is integer or
 * single-operation IEEE arithmetic: the device results equal a CPU restatement (tests/np_mirror_match.py) bit for bit.
 *
 * Definitions (this library's, stated where the reference leans on OpenCV or leaves behaviour undefined):
 *   - descriptors are 32 bytes (256 bits), keypoints are (x, y) float pairs = cv::KeyPoint::pt, at most CHIP_MATCH_MAX_KEYPOINTS per image;
 *   - brute-force match: for query i the train index of minimum Hamming distance, ties -> the LOWEST train index (the first minimum
 *     of a scan in index order, which is what OpenCV's batchDistance keeps); with n2 == 0 there are no matches (train_idx = distance = -1);
 *   - GMS: points normalised x / width, y / height in float; left and right grid 20 x 20; four passes with the left grid shifted by
 *     0 / half a cell in x / y / both (gms_matcher.h:143-182: floor(x * 20 [+ 0.5]) with the product rounded to float and the + 0.5 done
 *     in double; passes 2-4 reject a shifted coordinate < 1 or >= 20, pass 1 rejects >= 20), the right cell computed once (:184-189);
 *     per pass the 400 x 400 table of match counts per (left, right) cell, per left cell the right cell of maximal count (ties -> the
 *     lowest right index, gms_matcher.cpp:112-121), its score = sum of the table over the 3 x 3 neighbourhoods (same offset on both
 *     sides, neighbours outside either grid skipped), rejected iff score < 6.0 * sqrt(double(sum of the left neighbours' match counts)
 *     / number of neighbour pairs) (:128-146); a match is an inlier iff in ANY pass its (left, right) cell pair is the accepted pair of
 *     its left cell (:169-177).  A cell index outside [0, 400) -- keypoints outside their image, where the reference indexes out of
 *     bounds or compares against its -1 / -2 sentinels -- makes the match take no part in that pass (right cell: in any pass);
 *   - correspondence sets: pixel (int)u, (int)v (truncation, as PointFeatureMatching.cpp:121,180) of the H x W x 3 float image
 *     (CV_32FC3 layout); a point is dropped iff z < 0.1 || z > 25. with the float z widened to double (:122,:182) -- so z = 0.1f passes
 *     (0.1f > 0.1), and so does NaN, as in the reference; normalised coordinates = the first two rows of Kinv * (u, v, 1) in fp64,
 *     (r0 * u + r1 * v) + r2 without contraction; the caller supplies Kinv (the library does not invert).  A pixel outside its 3-D
 *     image (the reference would read out of bounds) drops the match from the sets that need that image; n_out_of_image counts the
 *     GMS inliers with at least one such pixel.
 * Not on chip_create_multi ctxs (CHIP_ERR_UNSUPPORTED, as chip_set_stream).  Work is enqueued on the ctx stream; one matching
 * thread per ctx next to the appender / tick threads, like the PnP caller (cerebro_node.cpp:509); chip_set_stream must not run
 * concurrently with these calls.  Scratch is allocated on first use and freed by chip_destroy.                                      */
#define CHIP_MATCH_MAX_KEYPOINTS 16384
#define CHIP_ORB_DESC_BYTES 32
int chip_build_has_match(void);     /* 1: this build of the library contains the stage (chip_info keeps its ABI 7 layout) */

int chip_orb_match(chip_ctx *ctx, const uint8_t *d1, int32_t n1, const uint8_t *d2, int32_t n2,
                   int32_t *train_idx /* n1 */, int32_t *distance /* n1 */);
/* kp*_xy: n* x 2 floats; matches as (query_idx[i] into kp1, train_idx[i] into kp2), CHIP_ERR_RANGE if one points outside;
 * inlier: n_matches bytes (0 / 1) in match order */
int chip_gms_filter(chip_ctx *ctx, const float *kp1_xy, int32_t n1, int32_t w1, int32_t h1,
                    const float *kp2_xy, int32_t n2, int32_t w2, int32_t h2,
                    const int32_t *query_idx, const int32_t *train_idx, int32_t n_matches,
                    uint8_t *inlier /* n_matches */, int32_t *n_inliers);

typedef struct {
    const uint8_t *desc;      /* n x CHIP_ORB_DESC_BYTES                                      */
    const float   *kp_xy;     /* n x 2, pixels                                                */
    int32_t        n;
    int32_t        width, height;   /* of the image AND of xyz                                */
    const float   *xyz;       /* height x width x 3 (CV_32FC3), the frame's 3-D image, host   */
} chip_match_frame;
typedef struct {
    int32_t n_matches_all;    /* matches_all.size()                  PointFeatureMatching.cpp:41  */
    int32_t n_matches_gms;    /* uv.cols() = pf_matches              Cerebro.cpp:1487,1505        */
    int32_t n_3d2d_ab;        /* world_point_uv.size()               Cerebro.cpp:1512             */
    int32_t n_3d2d_ba;        /* world_point_uv_d.size()             Cerebro.cpp:1566             */
    int32_t n_3d3d;           /* uv_X.size()                         Cerebro.cpp:1624             */
    int32_t n_out_of_image;
} chip_match_summary;
/* The whole stage for the pair (a, b): a's descriptors are the queries, b's the train set (gms_point_feature_matches(a, b, uv, uv_d),
 * Cerebro.cpp:1484).  One upload, nothing returns to the host in between but the six counts.  The five sets stay on the device,
 * attached to the ctx, until the next chip_match_pair. */
int chip_match_pair(chip_ctx *ctx, const chip_match_frame *a, const chip_match_frame *b, const double Kinv_rowmajor[9],
                    chip_match_summary *summary);
typedef struct {
    double  *uv, *uv_d;               /* n_matches_gms x 2: pixels of the GMS inliers in a and in b (the float keypoints as doubles) */
    double  *X_ab, *uvn_ab;           /* n_3d2d_ab x 3 / x 2: a's 3-D points, their normalised projections in b  */
    double  *X_ba, *uvn_ba;           /* n_3d2d_ba x 3 / x 2: b's 3-D points, their normalised projections in a  */
    double  *A_3d3d, *B_3d3d;         /* n_3d3d x 3 each                                                          */
    int32_t *match_query_idx, *match_train_idx;   /* n_matches_gms each: the GMS inliers as keypoint indices      */
} chip_match_sets_out;
/* host copies of what the last chip_match_pair left on the device; every pointer may be NULL; capacities = that summary's counts */
int chip_match_read_sets(chip_ctx *ctx, chip_match_sets_out *out);
/* The existing solvers on the device-resident sets, without the host round trip: results are those of chip_pnp_ransac /
 * chip_icp_ransac on the copied-out sets, bit for bit (same kernels, a device-pointer entry next to the host-pointer one).
 * which: CHIP_SET_AB = PNP(world_point_uv, feature_position_uv_d) -> b_T_a (Cerebro.cpp:1518), CHIP_SET_BA = the role-swapped call
 * -> a_T_b (:1572).  inlier_mask: that set's count bytes, may be NULL.  CHIP_ERR_BUSY before any chip_match_pair. */
enum { CHIP_SET_AB = 0, CHIP_SET_BA = 1 };
int chip_pnp_ransac_matched(chip_ctx *ctx, int32_t which, const chip_ransac_params *p, double T_colmajor[16], float *confidence,
                            uint8_t *inlier_mask, chip_ransac_summary *summary /* may be NULL */);
int chip_icp_ransac_matched(chip_ctx *ctx, const chip_ransac_params *p, double T_colmajor[16], float *confidence,
                            uint8_t *inlier_mask, chip_ransac_summary *summary /* may be NULL */);

/* ---- one query frame against B candidate frames (top-K lists, the clique policy, three queries per tick; a replay's backlog is a list
 * of PAIRS with a query frame each: chip_match_pairs_stored below): the
 * query frame is uploaded once and all B pairs share three launches -- hamming_match_split (grid: query blocks of 256 x train tiles of
 * 1024 x B; the partial minima of a (query, candidate) meet as the unsigned 64-bit key distance << 32 | train index, whose minimum is
 * the smallest distance and then the LOWEST train index, the tie rule above, whichever tile arrives first), gms_batch (one workgroup
 * per (grid type, candidate) on a table and a byte plane of its own) and pose_sets_batch (one workgroup per candidate; inlier = the
 * OR of its four planes).  The sets of all B candidates stay on the device in slabs of a->n rows.  ONE of them is "selected": the
 * one chip_match_read_sets, chip_pnp_ransac_matched and chip_icp_ransac_matched work on.
 * Status: B < 1 or a NULL pointer CHIP_ERR_INVALID_ARG; B > CHIP_MATCH_MAX_BATCH, a group ctx or a frame beyond chip_match_pair's
 * limits CHIP_ERR_UNSUPPORTED; j or cand[i] outside the last batch CHIP_ERR_RANGE; before any match CHIP_ERR_BUSY.  An empty
 * query frame or an empty candidate gives that candidate a zero summary, as chip_match_pair.  A failed call leaves nothing
 * selected.  chip_match_pair is this pipeline with one candidate.                                                                 */
#define CHIP_MATCH_MAX_BATCH 16            /* = the library's top-K bound */
int chip_build_has_match_batch(void);      /* 1 */
/* frame a against b[0..B): summary[j] and the five sets of candidate j are those of chip_match_pair(a, &b[j]) byte for byte.
 * One upload of a, one of each b[j], nothing returns to the host but the B x 6 counts.  Afterwards candidate 0 is selected. */
int chip_match_batch(chip_ctx *ctx, const chip_match_frame *a, const chip_match_frame *b, int32_t B,
                     const double Kinv_rowmajor[9], chip_match_summary *summary /* B */);
/* make candidate j of the last chip_match_batch the one that chip_match_read_sets, chip_pnp_ransac_matched and
 * chip_icp_ransac_matched work on.  After chip_match_pair there is one candidate, index 0. */
int chip_match_select(chip_ctx *ctx, int32_t j);
/* matches_all of candidate j (BFMatcher output before GMS): n1 = a->n train indices and distances, -1 / -1 where b[j].n == 0.
 * CHIP_ERR_BUSY unless the last match call of the ctx was a chip_match_batch[_stored] or a chip_match_pairs_stored (then j is the pair
 * index and n1 the n of THAT pair's query frame). */
int chip_match_batch_read_matches(chip_ctx *ctx, int32_t j, int32_t *train_idx, int32_t *distance);
/* P PnP estimations on device-resident sets in launches of up to 8 problems: problem i is set which[i] (CHIP_SET_AB / _BA)
 * of candidate cand[i], seed seeds[i] (NULL: p->seed).  status[i] is what chip_pnp_ransac_matched would return after
 * chip_match_select(cand[i]).  A set with fewer than 20 points gets CHIP_ERR_TOO_FEW_POINTS and is left out of the launch.
 * Its T is NaN, its confidence -1, its summary zero with best_hypothesis -1, and its mask is untouched.  The other problems
 * are bit-identical to the single call with that seed.  The call itself fails only on bad arguments or a HIP / allocation
 * error.  The selection is not changed.                                                                                   */
int chip_pnp_ransac_matched_batch(chip_ctx *ctx, int32_t P, const int32_t *cand, const int32_t *which,
                                  const chip_ransac_params *p, const uint64_t *seeds, double *T_colmajor /* P x 16 */,
                                  float *confidence /* P */, uint8_t *const *inlier_mask /* may be NULL */,
                                  chip_ransac_summary *summary /* P or NULL */, int32_t *status /* P */);
/* P ICP estimations on the device-resident 3-D / 3-D sets (A_3d3d, B_3d3d, n_3d3d) of candidates cand[i] of the last match call, read
 * in place, in ONE pair of launches on the ctx's ICP stream -- split into enqueue and collect so that they run underneath the PnP call
 * of the same candidates (nothing in them depends on it):
 *   _enqueue : status[i] is what chip_icp_ransac_matched would return after chip_match_select(cand[i]); a set with fewer than 20
 *              points gets CHIP_ERR_TOO_FEW_POINTS and is left out of the launch.  Problem i draws from seeds[i] (NULL: p->seed).
 *              cand may repeat and be in any order.  Returns without waiting.  With no runnable problem it still succeeds.
 *   _collect : waits and delivers the P answers.  A problem that ran is bit-identical to the single call with that seed; a left-out
 *              one has T = NaN, confidence -1, a zero summary with best_hypothesis -1 and an untouched mask.
 *   chip_icp_ransac_matched_batch = enqueue + collect.
 * The selection is not changed.  Status: before any match CHIP_ERR_BUSY; cand[i] outside the batch CHIP_ERR_RANGE; a group ctx or
 * P > CHIP_ICP_MAX_BATCH CHIP_ERR_UNSUPPORTED; P < 1 or a NULL pointer CHIP_ERR_INVALID_ARG; an ICP estimation already pending, or a
 * collect without a batch enqueue, CHIP_ERR_BUSY.  The sets outlive the kernels: chip_match_pair, chip_match_batch and
 * chip_match_batch_stored wait for the ICP stream first when a matched batch is pending; they still succeed and the batch stays
 * collectable (its results are in pinned memory by then).                                                                         */
int chip_icp_ransac_matched_batch_enqueue(chip_ctx *ctx, int32_t P, const int32_t *cand, const chip_ransac_params *p,
                                          const uint64_t *seeds, int32_t *status /* P */);
int chip_icp_ransac_matched_batch_collect(chip_ctx *ctx, double *T_colmajor /* P x 16 */, float *confidence /* P */,
                                          uint8_t *const *inlier_mask /* may be NULL */, chip_ransac_summary *summary /* P or NULL */);
int chip_icp_ransac_matched_batch(chip_ctx *ctx, int32_t P, const int32_t *cand, const chip_ransac_params *p, const uint64_t *seeds,
                                  double *T_colmajor /* P x 16 */, float *confidence /* P */, uint8_t *const *inlier_mask /* may be NULL */,
                                  chip_ransac_summary *summary /* P or NULL */, int32_t *status /* P */);

/* ---- frames kept on the device: the match stage without uploads.  chip_match_batch spends most of its time copying 3-D images of
 * which the sets read ONE pixel per keypoint, and the same keyframes come back call after call (three queries per tick, top-K lists
 * of neighbouring places, the query of now is a candidate later).  A frame is therefore PUT once under a caller-chosen 64-bit id
 * (DataNode / the data_map rank): its descriptors and keypoints stay on the device, the kernel frame_gather reads its 3-D points at
 * the keypoints, and the image is dropped.  chip_match_batch_stored then runs the pipeline above on stored frames by id.
 *
 * Definitions:
 *   - store layout: n_slots slots of slot_keypoints keypoints each, 1 <= slot_keypoints <= CHIP_MATCH_MAX_KEYPOINTS, 56 bytes per
 *     keypoint (32 descriptor, 8 keypoint, 16 point record): device memory = n_slots x slot_keypoints x 56 B, allocated once by
 *     chip_frame_store_reserve inside one pause of the resident scan (as the other buffers of the stage); rows never move after
 *     the reserve, as the DB segments.  The same two numbers again: a no-op.  Other numbers: allowed only while the store holds
 *     no frame (the store is then allocated anew), otherwise CHIP_ERR_BUSY.  n_slots < 1 or slot_keypoints out of range:
 *     CHIP_ERR_INVALID_ARG.  chip_destroy frees the store;
 *   - before any reserve: put, read and match_batch_stored return CHIP_ERR_BUSY, drop CHIP_ERR_RANGE, info reports 0 / 0 / 0;
 *   - chip_frame_put: the frame rules of chip_match_pair (NULL pointers CHIP_ERR_INVALID_ARG, sizes beyond its limits
 *     CHIP_ERR_UNSUPPORTED), then f->n > slot_keypoints CHIP_ERR_UNSUPPORTED (the caller keeps using host frames for such a frame).
 *     Descriptors and keypoints are uploaded into the slot, the image into a staging buffer (grown on demand, never part of the
 *     store); frame_gather runs on the ctx stream; n, width and height are kept with the slot.  The call returns when the copies
 *     and the kernel are complete: the caller's arrays are free again.  An id already stored is REPLACED in its own slot.  No free
 *     slot: CHIP_ERR_OOM -- nothing is evicted silently, eviction is the integrator's policy (chip_frame_drop).  A frame with
 *     n == 0 is stored.  A failed put leaves the store as it was and a failed replace keeps the old frame: every check and
 *     allocation precedes the first write to the slot.  The one exception is a HIP error AFTER the copies of a replace began
 *     (CHIP_ERR_HIP): the slot's rows are undefined then, and the id leaves the store;
 *   - point record: one float4 per keypoint.  The pixel is the one the sets use (truncation; (-1, w) maps into [0, w - 1]; NaN and
 *     everything else is outside).  Pixel in the image: (x, y, z, 1.0f), the three floats copied bit for bit from the image;
 *     otherwise (0, 0, 0, 0.0f).  The flag is a lane of its own because a NaN z passes the depth gate, as in the reference: no
 *     value of z can mean "outside";
 *   - chip_frame_drop: unknown id CHIP_ERR_RANGE; the slot is free for the next put.  Sets and keys an earlier match left stay
 *     valid (they live in the run's slabs, not in the store);
 *   - chip_frame_read: a read-back (tests, checkpoints): desc and kp_xy are the bytes that were put, pts the records; any pointer
 *     may be NULL; unknown id CHIP_ERR_RANGE;
 *   - chip_match_batch_stored: the status rules of chip_match_batch, and an unknown a_id or b_ids[j] CHIP_ERR_RANGE (nothing is
 *     selected, as after any failed call).  b_ids may repeat an id and may contain a_id.  An empty query frame or an empty
 *     candidate gives a zero summary.  summary[j], the ten arrays of chip_match_read_sets after chip_match_select(j) and
 *     chip_match_batch_read_matches(j) are byte for byte what chip_match_batch gives on the host frames that were put under those
 *     ids (pose_sets_stored_batch is pose_sets_batch with the records in place of the images; the other two kernels run as they
 *     are, on pointers into the store).  Afterwards candidate 0 is selected and chip_match_batch_read_matches answers;
 *     chip_match_select, chip_match_read_sets, chip_pnp_ransac_matched, chip_icp_ransac_matched, chip_pnp_ransac_matched_batch
 *     and chip_icp_ransac_matched_batch work on the result unchanged;
 *   - cost: no host-to-device copy of frame data; three launches and the B x 5 counts back.
 * Not on chip_create_multi ctxs (CHIP_ERR_UNSUPPORTED).  These calls belong to the one matching thread of the ctx and use the ctx
 * stream: a put is ordered before a later match.                                                                                   */
int chip_build_has_frame_store(void);      /* 1 */
int chip_frame_store_reserve(chip_ctx *ctx, int32_t n_slots, int32_t slot_keypoints);
int chip_frame_store_info(chip_ctx *ctx, int32_t *n_slots, int32_t *slot_keypoints, int32_t *n_frames /* each may be NULL */);
int chip_frame_put(chip_ctx *ctx, int64_t id, const chip_match_frame *f);
int chip_frame_drop(chip_ctx *ctx, int64_t id);
int chip_frame_read(chip_ctx *ctx, int64_t id, int32_t *n, int32_t *width, int32_t *height,
                    uint8_t *desc /* n x 32 */, float *kp_xy /* n x 2 */, float *pts /* n x 4 */);
int chip_match_batch_stored(chip_ctx *ctx, int64_t a_id, const int64_t *b_ids, int32_t B,
                            const double Kinv_rowmajor[9], chip_match_summary *summary /* B */);

/* ---- GMS with scale and rotation (ABI 7, additive): gms_matcher::GetInlierMask(mask, WithScale, WithRotation), the two booleans of
 * src/utils/PointFeatureMatching.cpp:52-53, as the bit set `modes`.  modes == 0 is the filter above, byte for byte; the plain form
 * keeps nothing of a candidate seen under a rolled camera or from half the distance.
 *
 * Definitions (restating src/utils/GMSMatcher/gms_matcher.{h,cpp}; everything not named here is as in the block above):
 *   - scales: index s = 0..4 has the ratios 1, 1/2, 1/sqrt(2), sqrt(2), 2 (gms_matcher.h:47); the right grid side is (int)(20 * ratio)
 *     with the product in double = 20, 10, 14, 28, 40 (:230-234), N_s = side^2 columns.  Without CHIP_GMS_WITH_SCALE only s = 0.  The
 *     left grid stays 20 x 20 with its four passes;
 *   - right cell at scale s: x = floorf(px * (float)side), y alike, index x + y * side (:185-190), no range check on x or y (x = width
 *     aliases into the next row, as at scale 0).  An index outside [0, N_s) -- where the reference leaves its tables -- has no right
 *     cell; non-finite or absurd coordinates have none either;
 *   - per (scale, pass): the 400 x N_s table, the left-cell counts and per non-empty left cell the first column of maximal count;
 *   - rotation types r = 1..8 (without CHIP_GMS_WITH_ROTATION: r = 1).  Number the 3 x 3 neighbourhood row-major 0..8 and take the
 *     ring of its eight outer positions clockwise from the top-left: (0, 1, 2, 5, 8, 7, 6, 3).  Pattern r pairs the left neighbour at
 *     ring position k with the right neighbour at ring position (k - (r - 1)) mod 8, and centre with centre; each step is 45 degrees,
 *     r = 1 is "same offset on both sides" (gms_matcher.h:12-44, used at gms_matcher.cpp:132-141).  A pair is skipped when either
 *     neighbour is outside its grid (left 20 x 20, right side x side).  score = sum of table[ll][rr] over the remaining pairs,
 *     threshold = 6.0 * sqrt(double(sum of cnt[ll]) / double(number of pairs)) over THE SAME pairs -- at a border of either grid both
 *     depend on the rotation; the left cell is rejected iff (double)score < threshold;
 *   - mask of (s, r): the OR over the four passes of "my cell pair is the accepted pair of my left cell";
 *   - choice: s ascending and r ascending inside it, the first (s, r) whose inlier count is strictly greater than every earlier one,
 *     starting from 0 (gms_matcher.cpp:19-33,38-48,54-66).  If every count is 0 nothing is chosen: the mask is all zero, n_inliers 0,
 *     scale -1, rotation 0 (the reference leaves the caller's vector untouched, i.e. empty);
 *   - chip_gms_choice.counts[s][r - 1]: the inlier count of (s, r), -1 for the combinations the modes did not try.  modes == 0:
 *     scale 0, rotation 1, counts[0][0] = the plain count.  No matches at all (n_matches == 0, an empty query frame or candidate):
 *     scale -1, rotation 0, 0 for the combinations the modes try;
 *   - kernels: gms_grid_modes, one workgroup per (scale, pass, candidate), builds table and column search once and scores the
 *     400 x 8 (left cell, rotation) items; gms_mode_select, one workgroup per candidate, counts the hypotheses, chooses, and writes the
 *     winner's mask where gms_batch writes its planes, so pose_sets_batch and everything behind run unchanged.  Four launches per
 *     batch, whatever B, the scales and the rotations;
 *   - memory: the tables are [B][S][4][400][N_s] int32 -- 2.56 MB per candidate without scale, 19.7 MB with (315 MB at B = 16) --
 *     plus S x 4 bytes per match, reserved on the first call with modes != 0 inside one pause of the resident scan.  A process that
 *     never passes modes != 0 allocates nothing of it.
 * Statuses, limits, selection and state are those of the calls they extend; a bit outside CHIP_GMS_WITH_SCALE | CHIP_GMS_WITH_ROTATION
 * is CHIP_ERR_INVALID_ARG.  Afterwards candidate 0 is selected, and chip_match_select, chip_match_read_sets,
 * chip_match_batch_read_matches, chip_pnp_ransac_matched[_batch] and chip_icp_ransac_matched[_batch[_enqueue]] work as after
 * chip_match_batch.  choice may be NULL.                                                                                            */
enum { CHIP_GMS_WITH_SCALE = 1, CHIP_GMS_WITH_ROTATION = 2 };
typedef struct {
    int32_t scale;            /* 0..4, -1: nothing chosen                                     */
    int32_t rotation;         /* 1..8,  0: nothing chosen                                     */
    int32_t n_inliers;
    int32_t counts[5][8];
} chip_gms_choice;
int chip_build_has_gms_modes(void);        /* 1 */
int chip_gms_filter_modes(chip_ctx *ctx, const float *kp1_xy, int32_t n1, int32_t w1, int32_t h1,
                          const float *kp2_xy, int32_t n2, int32_t w2, int32_t h2,
                          const int32_t *query_idx, const int32_t *train_idx, int32_t n_matches, uint32_t modes,
                          uint8_t *inlier /* n_matches */, int32_t *n_inliers, chip_gms_choice *choice /* or NULL */);
int chip_match_batch_modes(chip_ctx *ctx, const chip_match_frame *a, const chip_match_frame *b, int32_t B,
                           const double Kinv_rowmajor[9], uint32_t modes, chip_match_summary *summary /* B */,
                           chip_gms_choice *choice /* B or NULL */);
int chip_match_batch_stored_modes(chip_ctx *ctx, int64_t a_id, const int64_t *b_ids, int32_t B, const double Kinv_rowmajor[9],
                                  uint32_t modes, chip_match_summary *summary /* B */, chip_gms_choice *choice /* B or NULL */);

/* ---- a list of (query, candidate) pairs on stored frames (ABI 7, additive).  The batched calls above share ONE query frame; a replay's
 * backlog does not have that shape: the reference's consumer thread walks foundLoops[prev .. new) (src/Cerebro.cpp:1224-1232) and every
 * entry is a pair (t_curr, t_prev) with a current frame of its own.  chip_match_pairs_stored runs P such pairs in the launches of ONE
 * batch, so that the batched PnP and ICP calls reach a backlog too.
 *
 * Definitions:
 *   - for every j, summary[j], choice[j], the ten arrays of chip_match_read_sets after chip_match_select(j) and
 *     chip_match_batch_read_matches(j) are byte for byte what chip_match_batch_stored_modes(ctx, a_ids[j], &b_ids[j], 1, Kinv, modes, ..)
 *     gives (modes == 0: chip_match_batch_stored).  chip_match_batch_read_matches(j) delivers the n of frame a_ids[j] entries;
 *   - a_ids may repeat, b_ids may repeat, a pair may be (x, x).  An empty query frame or an empty candidate gives that pair a zero
 *     summary and the "nothing chosen" choice and disturbs no other pair;
 *   - kernels: hamming_match_pairs (grid: query blocks of 256 over the widest query frame x train tiles of 1024 x P; a workgroup
 *     beyond its own pair's query frame or candidate leaves at once), pairs_gms (or pairs_grid_modes + pairs_mode_select) and
 *     pose_sets_stored_pairs: the bodies of the batch kernels with the pair's own query frame, which travels next to its candidate
 *     in the kernel arguments.  Three launches (four with modes != 0) whatever P and however many distinct query frames.  Keys,
 *     planes and slabs are rows of max_j n(a_ids[j]) per pair;
 *   - afterwards pair 0 is selected and chip_match_batch_read_matches answers; chip_match_select, chip_match_read_sets,
 *     chip_pnp_ransac_matched[_batch] and chip_icp_ransac_matched[_batch[_enqueue / _collect]] work on the result unchanged, with
 *     cand[i] the pair index.  A pending matched ICP batch is waited for first, as in the other runs;
 *   - status: P < 1 or a NULL a_ids / b_ids / Kinv / summary, or a modes bit outside the two defined, CHIP_ERR_INVALID_ARG;
 *     P > CHIP_MATCH_MAX_PAIRS or a group ctx CHIP_ERR_UNSUPPORTED; before any chip_frame_store_reserve CHIP_ERR_BUSY; an unknown id
 *     on either side CHIP_ERR_RANGE (nothing is selected afterwards, as after any failed call).
 * There is no pair list on host frames: it would upload a query frame per pair, which the store exists to avoid.  A backlog longer
 * than CHIP_MATCH_MAX_PAIRS is the caller's loop.                                                                                   */
#define CHIP_MATCH_MAX_PAIRS CHIP_MATCH_MAX_BATCH      /* 16 */
int chip_build_has_match_pairs(void);      /* 1 */
int chip_match_pairs_stored(chip_ctx *ctx, const int64_t *a_ids, const int64_t *b_ids, int32_t P, const double Kinv_rowmajor[9],
                            uint32_t modes, chip_match_summary *summary /* P */, chip_gms_choice *choice /* P or NULL */);

/* ---- a frame from its disparity map: the 3-D points computed on the device (ABI 7, additive).  chip_frame_put wants the frame's
 * complete CV_32FC3 3-D image, of which frame_gather reads one pixel per keypoint; the reference makes that image on the host, over
 * all w x h pixels, with StereoGeometry::disparity_to_3DPoints (src/utils/CameraGeometry.cpp:459-524; the consumer thread reaches it
 * through :728-742 from src/Cerebro.cpp:1459,1472), and it is six times the bytes of cv::StereoBM's CV_16SC1 disparity (:81,:416).
 * That function is plain arithmetic on five entries of Q, so it is restated here and computed where it is used.
 *
 * Definitions (restating CameraGeometry.cpp:485-523):
 *   - Q_rowmajor: the 4 x 4 double Q (cv::stereoRectify), row-major.  Five entries count: Q03, Q13, Q23, Q32, Q33 = (0,3), (1,3),
 *     (2,3), (3,2), (3,3), each narrowed to float ON THE HOST (the CV_64F branch, :494-498; a CV_32F Q widened to double narrows back
 *     exactly).  Every other entry is ignored (:484);
 *   - disparity: height x width, dense rows, CHIP_DISP_S16 (CV_16SC1, StereoBM / SGBM raw: 16 x the disparity in pixels) or
 *     CHIP_DISP_F32 (CV_32FC1 in the same units).  d = the value as a float; an int16 converts exactly (convertTo, :472-473);
 *   - pw = (float)(1.0 / ((((double)d / 16.0) * (double)Q32 + (double)Q33) + 1e-6)): every operation in fp64 in that order, an IEEE
 *     fp64 divide, ONE narrowing to float at the end (:511).  d / 16 * Q32 is exact in fp64 (24 x 24 significant bits);
 *   - pixel (row i, column j): x = ((float)j + Q03) * pw, y = ((float)i + Q13) * pw, z = Q23 * pw, in fp32 without contraction
 *     (:520-522; the reference is built without FMA);
 *   - a NaN result is a NaN: its sign and payload are NOT defined (x86 and gfx950 differ there).  Everything else is bit for bit
 *     what the reference's loop gives, infinities and signed zeros included.
 *   - chip_frame_put_disparity: chip_frame_put with the disparity in the place of f->xyz.  Every rule of chip_frame_put holds
 *     (statuses in its order, replace in the own slot, n == 0 is stored, CHIP_ERR_OOM when the store is full, n > slot_keypoints
 *     and a group ctx CHIP_ERR_UNSUPPORTED, CHIP_ERR_BUSY before a reserve, a failed put leaves the store as it was, the call
 *     returns when the copies and the kernel are complete); in addition an unknown disp_type or a NULL Q_rowmajor is
 *     CHIP_ERR_INVALID_ARG.  The disparity goes into the staging buffer of chip_frame_put (bytes; grown on demand, a put never
 *     shrinks it).  The kernel disparity_gather, one thread per keypoint, takes the pixel frame_gather takes and writes the record
 *     (x, y, z, 1.0f) of that pixel's disparity, otherwise (0, 0, 0, 0.0f).  Record layout and every reader of it are unchanged: a
 *     frame put this way and the same frame put through chip_frame_put with the image of chip_disparity_to_xyz are
 *     indistinguishable afterwards;
 *   - chip_disparity_to_xyz: the dense out3D of :482-524 into host memory, for callers that stay on host frames (chip_match_batch,
 *     frames larger than a slot).  Kernel disparity_to_xyz: a thread takes four consecutive pixels of a row -- one 8- or 16-byte
 *     load and three 16-byte stores where the row position and the pointers allow, pixel by pixel otherwise.  Needs no frame
 *     store; runs on the ctx stream, serialised with the other calls of the stage.  NULL ctx / disparity / Q_rowmajor / xyz, a
 *     size < 1 or an unknown disp_type CHIP_ERR_INVALID_ARG; a side beyond the image limit of chip_match_pair or a group ctx
 *     CHIP_ERR_UNSUPPORTED.  The valid-point matrix of the reference (fill_eigen_matrix, :551-618) is not built.               */
enum { CHIP_DISP_S16 = 0, CHIP_DISP_F32 = 1 };
int chip_build_has_disparity(void);        /* 1 */
int chip_frame_put_disparity(chip_ctx *ctx, int64_t id, const uint8_t *desc /* n x 32 */, const float *kp_xy /* n x 2 */, int32_t n,
                             int32_t width, int32_t height, const void *disparity /* height x width, dense rows */,
                             int32_t disp_type, const double Q_rowmajor[16]);
int chip_disparity_to_xyz(chip_ctx *ctx, const void *disparity /* height x width */, int32_t disp_type, int32_t width, int32_t height,
                          const double Q_rowmajor[16], float *xyz /* height x width x 3, host */);

/* ---- a frame from its rectified stereo pair: the block matcher on the device, at the keypoints (ABI 7, additive).  The disparity map
 * chip_frame_put_disparity takes is made by cv::StereoBM::create(64, 21) on the rectified 8-bit pair (src/utils/CameraGeometry.cpp:81,
 * 416; twice per candidate from src/Cerebro.cpp:1459,1472): 64 disparities x a 21 x 21 window at every pixel on a host core, of
 * which the stage reads one pixel per keypoint.  A block matcher's answer at a pixel depends on a small 8-bit neighbourhood only, and
 * the two images are exactly the bytes of the int16 map (2 w h), so the disparity is computed here, at the keypoints, on the put.
 *
 * THE DEFINITION IS THIS PROJECT'S OWN, modelled on cv::StereoBM with PREFILTER_XSOBEL.  OpenCV's source is not part of this project,
 * so parity against it is UNPINNED (DESIGN.md 6 lists the known departures).  All arithmetic is int32.
 *   - parameters (chip_stereo_bm_params, five int32_t, 20 bytes; defaults = StereoBM::create(64, 21)); a value outside is
 *     CHIP_ERR_UNSUPPORTED:  num_disparities 64 (16, 32, 48, 64);  block_size 21 (odd, 5 .. 21);  prefilter_cap 31 (1 .. 63);
 *     texture_threshold 10 (>= 0);  uniqueness_ratio 15 (0 .. 100, 0 = off).  Minimum disparity 0; no speckle filter, no
 *     left-right check (StereoBM's defaults; the reference sets neither).  Below r = block_size / 2, nd = num_disparities,
 *     cap = prefilter_cap;
 *   - prefilter of an image I (uint8, h x w, dense rows) into P: for 1 <= x <= w - 2
 *       v = (I[y-][x+1] - I[y-][x-1]) + 2 (I[y][x+1] - I[y][x-1]) + (I[y+][x+1] - I[y+][x-1]),  P[y][x] = min(max(v, -cap), cap) + cap
 *     with reflected rows (y- = y - 1, row -1 is row 1; y+ = y + 1, row h is row h - 2; with h == 1 both are row 0); columns 0 and
 *     w - 1: P = cap.  P lies in [0, 2 cap];
 *   - defined pixels: r <= y <= h - 1 - r and nd - 1 + r <= x <= w - 1 - r (every byte of every window inside the images).  Every
 *     other pixel has the value -16 = (minDisparity - 1) * 16, StereoBM's "no disparity";
 *   - at a defined pixel, windows over dy, dx in [-r, r]:  T = sum |PL[y+dy][x+dx] - cap|;  SAD(d) = sum |PL[y+dy][x+dx] -
 *     PR[y+dy][x+dx-d]|, d = 0 .. nd - 1;  m = min SAD;  D = the LARGEST d with SAD(d) == m;
 *       texture:    T < texture_threshold -> -16;
 *       uniqueness: (ratio > 0) thresh = m + m * ratio / 100 (integer division); some d with |d - D| > 1 and SAD(d) <= thresh -> -16;
 *       sub-pixel:  p = SAD(D - 1), n = SAD(D + 1); at D == 0 both are SAD(1), at D == nd - 1 both are SAD(nd - 2);
 *                   q = p + n - 2 m + |p - n|;  value = (D * 256 + (q != 0 ? (p - n) * 256 / q : 0) + 15) >> 4, `/` truncating
 *                   toward zero (the sum is never negative): an int16 in sixteenths of a pixel, exactly CHIP_DISP_S16;
 *   - chip_stereo_bm: the dense map into host memory (kernels bm_prefilter, bm_dense: one wave per pixel, the definition made
 *     callable, not a hot path).  NULL ctx / left / right / disparity or a size < 1 CHIP_ERR_INVALID_ARG; a side beyond the image
 *     limit of chip_match_pair, a group ctx or a refused parameter CHIP_ERR_UNSUPPORTED.  Images too small to hold a defined pixel
 *     are no error: the map is all -16.  Needs no frame store; runs on the ctx stream, serialised with the other calls of the stage;
 *   - chip_frame_put_stereo: chip_frame_put_disparity with the pair in the place of the map.  Every rule of chip_frame_put holds
 *     (statuses in its order, replace in the own slot, n == 0 is stored, CHIP_ERR_OOM when the store is full, n > slot_keypoints
 *     and a group ctx CHIP_ERR_UNSUPPORTED, CHIP_ERR_BUSY before a reserve, a failed put leaves the store as it was, the call
 *     returns when the copies and the kernels are complete); in addition a NULL left / right / Q_rowmajor is CHIP_ERR_INVALID_ARG
 *     and a refused parameter CHIP_ERR_UNSUPPORTED, both before anything touches the ctx's device.  The two images go into the
 *     staging buffer of chip_frame_put (2 w h bytes: what the int16 map takes), bm_prefilter writes the prefiltered pair into a
 *     buffer of its own, and bm_keypoints -- one wave per keypoint, lane = disparity, four absolute byte differences per
 *     instruction -- takes the pixel frame_gather takes, computes its disparity by the definition and writes the record
 *     (x, y, z, 1.0f) of point_of_disparity of that value, otherwise (0, 0, 0, 0.0f).  A frame put this way and the same frame put
 *     through chip_frame_put_disparity with CHIP_DISP_S16 and the map of chip_stereo_bm are indistinguishable afterwards.         */
typedef struct {
    int32_t num_disparities;     /* 64: 16, 32, 48 or 64 */
    int32_t block_size;          /* 21: odd, 5 .. 21 */
    int32_t prefilter_cap;       /* 31: 1 .. 63 */
    int32_t texture_threshold;   /* 10: >= 0 */
    int32_t uniqueness_ratio;    /* 15: 0 .. 100, 0 = off */
} chip_stereo_bm_params;
void chip_stereo_bm_params_default(chip_stereo_bm_params *p);
int chip_build_has_stereo_bm(void);        /* 1 */
int chip_stereo_bm(chip_ctx *ctx, const uint8_t *left, const uint8_t *right /* height x width each, dense rows */, int32_t width,
                   int32_t height, const chip_stereo_bm_params *p /* NULL: the defaults */, int16_t *disparity /* height x width, host */);
int chip_frame_put_stereo(chip_ctx *ctx, int64_t id, const uint8_t *desc /* n x 32 */, const float *kp_xy /* n x 2 */, int32_t n,
                          int32_t width, int32_t height, const uint8_t *left, const uint8_t *right /* height x width each */,
                          const chip_stereo_bm_params *p /* NULL: the defaults */, const double Q_rowmajor[16]);

/* ---- ORB keypoint detection on the device: FAST-9, Harris ranking, up to 8 pyramid levels (ABI 7, additive).  The kp_xy every
 * chip_frame_put* takes is the detector half of cv::ORB::create(5000) with setFastThreshold(0) on the rectified left image
 * (src/utils/PointFeatureMatching.cpp:16-22, on both frames of every candidate).  chip_orb_detect is that half: the pyramid, the FAST
 * score, the Harris ranking with per-level quotas and the patch moments the orientation is made of.  The descriptor half (blur,
 * steered BRIEF) is built as well: "ORB descriptors on the device", below (chip_orb_detect_describe).
 *
 * THE DEFINITION IS THIS PROJECT'S OWN, modelled on cv::ORB::detect with HARRIS_SCORE.  OpenCV's source is not part of this project,
 * so parity against it is UNPINNED (DESIGN.md 6 lists the known departures).  All image arithmetic is integer; the device results
 * equal a CPU restatement (tests/np_mirror_orb_detect.py) bit for bit.
 *   - parameters (chip_orb_params, four int32_t, 16 bytes); a value outside is CHIP_ERR_UNSUPPORTED:  n_features 5000
 *     (1 .. CHIP_MATCH_MAX_KEYPOINTS);  n_levels 8 (1 .. CHIP_ORB_MAX_LEVELS; the scale factor is fixed at 1.2);  fast_threshold 0
 *     (PointFeatureMatching.cpp:18; 0 .. 255);  border 31 (ORB's edgeThreshold; 16 .. 64);
 *   - levels: s_0 = 1.0, s_l = s_(l-1) * 1.2 in double; w_l = (int)floor(w / s_l + 0.5), h_l alike (a level may have a side of 0: it
 *     holds nothing);
 *   - quotas: f = 1.0 / 1.2; g = 1.0 multiplied by f n_levels times (no pow); nd = n_features * (1 - f) / (1 - g); for l < n_levels - 1
 *     quota_l = min((int)floor(nd + 0.5), n_features - sum), then nd *= f; the last level gets n_features - sum: the quotas sum to
 *     n_features (without the min the rounding gives 8 for n_features = 7 on 8 levels, the one such case up to 16384).  A level
 *     without a detection area keeps its quota: nothing is redistributed;
 *   - chip_orb_plan: exactly the table a launch uses, without a ctx or a device: width, height, quota, the detection rectangle
 *     border <= x <= w_l - 1 - border, border <= y <= h_l - 1 - border as x0, y0, x1, y1 (an empty one is 0, 0, -1, -1) and s_l.
 *     Entries from n_levels on are zero.  The statuses are those of chip_orb_detect for width, height and p;
 *   - pyramid: level 0 is the image.  Level l is made from level l - 1 by fixed-point bilinear sampling at pixel centres:
 *     X = ((2x + 1) * w_(l-1) * 1024) / w_l - 1024 (a 64-bit integer division; units of 1/2048 pixel), clamped to
 *     [0, (w_(l-1) - 1) * 2048]; x0 = X >> 11, a = X & 2047, x1 = min(x0 + 1, w_(l-1) - 1); the same in y with b;
 *     value = (I[y0][x0] (2048 - a)(2048 - b) + I[y0][x1] a (2048 - b) + I[y1][x0] (2048 - a) b + I[y1][x1] a b + (1 << 21)) >> 22;
 *   - FAST score S, at every pixel at least 3 from each edge of its level.  The ring k = 0..15 as (dx, dy):
 *       (0,-3) (1,-3) (2,-2) (3,-1) (3,0) (3,1) (2,2) (1,3) (0,3) (-1,3) (-2,2) (-3,1) (-3,0) (-3,-1) (-2,-2) (-1,-3)
 *     b = the maximum over the 16 cyclic arcs of 9 consecutive ring pixels of the minimum over the arc of I_k - I_p, d = the same with
 *     I_p - I_k, S = max(b, d) - 1 in [-256, 254].  A pixel is a corner at threshold t iff S >= t; a flat region has S = -1.  Where S
 *     is not defined the score plane holds -256;
 *   - candidates: the pixels of the detection rectangle with S >= fast_threshold and S strictly greater than the S of all eight
 *     neighbours (a plateau of equal scores keeps nothing);
 *   - Harris key: Ix = 2 (I[y][x+1] - I[y][x-1]) + (I[y-1][x+1] - I[y-1][x-1]) + (I[y+1][x+1] - I[y+1][x-1]), Iy = Ix transposed;
 *     a = sum Ix^2, bb = sum Iy^2, c = sum Ix Iy over the 7 x 7 block centred on the candidate (int32); R = 25 (a bb - c c) -
 *     (a + bb)^2 exactly in int64: Harris with k = 0.04, times 25;
 *   - selection: per level the quota_l candidates of largest R, or all if there are fewer; ties go to the lower raster index
 *     y w_l + x.  Output order: level ascending, raster order inside a level.  level_counts: the kept count per level (0 from
 *     n_levels on);
 *   - moments: m10 = sum u I, m01 = sum v I over v in [-15, 15], u in [-umax(|v|), umax(|v|)],
 *     umax[0..15] = 15 15 15 15 14 14 14 13 13 12 11 10 9 8 6 3 (749 pixels), int32.  The caller's orientation is
 *     atan2(m01, m10); the library computes no angle;
 *   - record (chip_orb_keypoint, 32 bytes): response = R; x, y = (float)((double)x_level * s_l), (float)((double)y_level * s_l);
 *     m10, m01; x_level, y_level, level; zero = 0;
 *   - kernels: orb_pyramid (one launch per level above 0: a level needs the one before), then four launches whatever n_levels, with
 *     the level table in the kernel arguments and the level on a grid axis: orb_fast_score (LDS tile of 128 x 16 pixels with a halo,
 *     eight pixels per thread, one 16-byte store each), orb_candidates (one workgroup per strip of two rows of the detection
 *     rectangle: ordered compaction of the strict maxima, Harris for those only), orb_select (one workgroup per level: radix select
 *     of the quota_l-th largest R over LDS histograms, ordered compaction) and orb_moments (one wave per kept keypoint, two 16-byte
 *     stores per record).  Counts and thresholds stay in device memory; one device-to-host copy of records and counts ends the call;
 *   - statuses, all decided before anything touches the device: NULL ctx / image / kp / n, a side < 1 or capacity < n_features
 *     CHIP_ERR_INVALID_ARG; a parameter outside its range, a side above CHIP_ORB_MAX_SIDE or a group ctx CHIP_ERR_UNSUPPORTED.  An
 *     image too small to hold a detection area is no error: *n = 0;
 *   - chip_debug_orb_level: the pyramid level (h_l x w_l, dense rows) and the FAST score plane (h_l x w_l int16) the last
 *     chip_orb_detect of the ctx left behind; either pointer may be NULL.  CHIP_ERR_BUSY if there is none, CHIP_ERR_RANGE for a
 *     level that call did not have.  It launches nothing.
 * Needs no frame store; runs on the ctx stream, serialised with the other calls of the stage.  The device buffers are grown on first
 * use or on a larger image inside one pause of the resident scan; a process that never calls it allocates nothing.                 */
#define CHIP_ORB_MAX_LEVELS 8
#define CHIP_ORB_MAX_SIDE 4096
typedef struct {
    int32_t n_features;          /* 5000: 1 .. CHIP_MATCH_MAX_KEYPOINTS */
    int32_t n_levels;            /* 8: 1 .. CHIP_ORB_MAX_LEVELS; scale factor fixed at 1.2 */
    int32_t fast_threshold;      /* 0 (PointFeatureMatching.cpp:18): 0 .. 255 */
    int32_t border;              /* 31 (ORB's edgeThreshold): 16 .. 64 */
} chip_orb_params;
typedef struct {
    int64_t response;            /* R, exact */
    float x, y;                  /* level-0 coordinates: (float)((double)x_level * s_l) */
    int32_t m10, m01;            /* patch moments */
    uint16_t x_level, y_level, level, zero;
} chip_orb_keypoint;
typedef struct {
    int32_t width, height, quota, x0, y0, x1, y1;
    double scale;
} chip_orb_level;
void chip_orb_params_default(chip_orb_params *p);
int chip_build_has_orb_detect(void);       /* 1 */
int chip_orb_plan(int32_t width, int32_t height, const chip_orb_params *p /* NULL: the defaults */, chip_orb_level levels[8]);
int chip_orb_detect(chip_ctx *ctx, const uint8_t *image /* height x width, dense rows */, int32_t width, int32_t height,
                    const chip_orb_params *p /* NULL: the defaults */, chip_orb_keypoint *kp, int32_t capacity, int32_t *n,
                    int32_t level_counts[8] /* may be NULL */);
int chip_debug_orb_level(chip_ctx *ctx, int32_t level, uint8_t *image_out /* h_l x w_l */, int16_t *score_out /* h_l x w_l */);

/* ---- ORB descriptors on the device: blur, 32 orientation bins, steered BRIEF (ABI 7, additive).  chip_orb_detect_describe is
 * detectAndCompute in one call (src/utils/PointFeatureMatching.cpp:21-22); chip_frame_put_orb_stereo puts a frame into the store from
 * its rectified 8-bit pair and nothing else: 2 w h bytes go up, one count comes down.
 *
 * THE DEFINITION IS THIS PROJECT'S OWN, all-integer, restated in tests/np_mirror_orb_describe.py (which the device equals bit for
 * bit) and UNPINNED against OpenCV: the pattern below is not cv::ORB's learned table.  Descriptors are only ever compared with
 * descriptors made by the same code; an integrator who must keep OpenCV's bits keeps orb->compute.
 *   - blurred level: for every pyramid level l, B_l has the level's size.  With g = 9 17 24 28 24 17 9 (sum 128):
 *       H[y][x] = sum_{i=-3..3} g[i+3] I[y][clamp(x + i, 0, w_l - 1)]
 *       B[y][x] = (sum_{j=-3..3} g[j+3] H[clamp(y + j, 0, h_l - 1)][x] + 8192) >> 14      in 0 .. 255
 *     The clamps make the plane defined everywhere; with border >= 16 no descriptor reads a clamped tap (reach, below);
 *   - orientation bin: CHIP_ORB_BINS = 32 bins of 11.25 degrees.  C[k] = round(16384 cos(2 pi k / 32)), S[k] alike, as literals:
 *       C[0..8] = 16384 16069 15137 13623 11585 9102 6270 3196 0      S[0..8] = 0 3196 6270 9102 11585 13623 15137 16069 16384
 *       C[(k + 8) mod 32] = -S[k], S[(k + 8) mod 32] = C[k]           (the nearest defining product lies 0.037 from a rounding half)
 *     bin(m10, m01) = the k that maximises m10 C[k] + m01 S[k], computed in int64, ties to the lowest k: (0, 0) gives 0,
 *     (3196, 315) ties bins 0 and 1 exactly and gives 0.  No float, no atan2.  chip_orb_bin is this function on the host;
 *   - pattern: 256 pairs (x1, y1, x2, y2) from a generator.  State s = 0x4F52425F42524945; a draw is
 *     s = s * 6364136223846793005 + 1442695040888963407 (mod 2^64), value (s >> 33) % 11 - 5; a coordinate is the sum of three
 *     draws; an attempt draws x1, y1, x2, y2 in that order (always 12 draws) and is rejected if either point has x^2 + y^2 > 169,
 *     if (x1 - x2)^2 + (y1 - y2)^2 < 9, or if the pair, in either order, was already accepted.  303 attempts give the 256 pairs;
 *     pairs 0, 1, 2 are (-6,-10,-4,0) (-7,-3,2,-5) (-1,-5,5,3), pair 255 is (-9,-2,-2,-6); sha256 of the 1024 int8 bytes
 *     [pair][x1,y1,x2,y2] is 0a170a01e941c47e3dc21a502fbec04104b548ddedf269114180a0504526a179;
 *   - steered table: T[k][pair] = (rx1, ry1, rx2, ry2), rx = (x C[k] - y S[k] + 8192) >> 14, ry = (x S[k] + y C[k] + 8192) >> 14
 *     (arithmetic shifts).  Every entry lies in -13 .. 13, no product hits an exact half, no pair collapses onto one pixel under any
 *     bin, and T[k + 8] is exactly T[k] turned by 90 degrees, (rx, ry) -> (-ry, rx): an image turned by a quarter turn gives the same
 *     descriptors.  sha256 of the 32768 int8 bytes [k][pair][rx1,ry1,rx2,ry2] is
 *     489d64ba52aef79c6fa46391b51cc6fe2e3764aa946f9283360aca763ba5969f.  The library builds both tables once, in plain host C++ from
 *     the generator, and uploads them on first use; chip_orb_pattern hands them out (either pointer may be NULL, both NULL is
 *     CHIP_ERR_INVALID_ARG; no ctx, no device);
 *   - descriptor: a keypoint has level l, position (x, y) = (x_level, y_level) and bin k = bin(m10, m01).  Bit p is 1 iff
 *     B_l[y + ry1][x + rx1] < B_l[y + ry2][x + rx2]; byte j holds the pairs 8j .. 8j + 7, LSB first: CHIP_ORB_DESC_BYTES = 32 bytes;
 *   - reach: the taps go +-13 and the blur +-3 beyond them; the detector's border is at least 16, so every read is inside the level;
 *   - kernels, both after orb_moments on the same stream and only in a describing call: orb_blur (all levels in one launch, the level
 *     on a grid axis; rows read as whole dwords into an LDS tile of 128 x 32 pixels with a halo of 3, 16-bit horizontal sums, 16-byte
 *     stores) and orb_describe (one wave per kept keypoint: the bin from the record's moments, the lane's four pairs in one 16-byte
 *     load, eight byte gathers, four ballots, two 16-byte stores; its output pointers are arguments);
 *   - chip_orb_detect_describe: the records and counts are byte for byte those of chip_orb_detect on the same input, desc[i] belongs
 *     to kp[i]; desc holds capacity x 32 bytes, of which the first *n x 32 are written.  Statuses: those of chip_orb_detect, and
 *     CHIP_ERR_INVALID_ARG for a NULL desc.  One device-to-host copy more than chip_orb_detect, for the descriptors;
 *   - chip_debug_orb_blur: the blurred plane (h_l x w_l, dense rows) of the last describing call of the ctx.  CHIP_ERR_BUSY if there
 *     is none (also after a plain chip_orb_detect), CHIP_ERR_RANGE for a level that call did not have.  It launches nothing;
 *   - chip_frame_put_orb_stereo: detect + describe on `left`, where the pair is staged for the block matcher; orb_describe writes
 *     the descriptors and the records' (x, y) straight into the slot's rows; then bm_prefilter and bm_keypoints as in
 *     chip_frame_put_stereo.  The only copy back is the eight kept counts, giving *n; each image crosses the bus once.  The frame is
 *     indistinguishable from chip_orb_detect_describe -> chip_frame_put_stereo with kp_xy from the records.  All statuses are decided
 *     before the device is touched: the checks of chip_orb_detect (NULL left / right / Q / n: CHIP_ERR_INVALID_ARG) and of
 *     chip_frame_put_stereo's parameters; a group ctx CHIP_ERR_UNSUPPORTED; no reserve CHIP_ERR_BUSY; n_features > slot_keypoints
 *     CHIP_ERR_UNSUPPORTED (the slot must hold whatever is kept); a full store CHIP_ERR_OOM.  The replace, failure and id rules are
 *     those of chip_frame_put; an image that keeps nothing is stored as an empty frame (*n = 0).                                    */
#define CHIP_ORB_BINS 32
int chip_build_has_orb_describe(void);     /* 1 */
int chip_orb_bin(int32_t m10, int32_t m01);
int chip_orb_pattern(int8_t pattern[1024] /* may be NULL */, int8_t steered[32768] /* may be NULL */);
int chip_orb_detect_describe(chip_ctx *ctx, const uint8_t *image /* height x width, dense rows */, int32_t width, int32_t height,
                             const chip_orb_params *p /* NULL: the defaults */, chip_orb_keypoint *kp, int32_t capacity, int32_t *n,
                             int32_t level_counts[8] /* may be NULL */, uint8_t *desc /* capacity x 32 */);
int chip_debug_orb_blur(chip_ctx *ctx, int32_t level, uint8_t *out /* h_l x w_l */);
int chip_frame_put_orb_stereo(chip_ctx *ctx, int64_t id, int32_t width, int32_t height, const uint8_t *left, const uint8_t *right,
                              const chip_orb_params *orb /* NULL: the defaults */, const chip_stereo_bm_params *bm /* NULL: the defaults */,
                              const double Q_rowmajor[16], int32_t *n);

/* ---- a frame from its raw stereo pair: rectification on the device (ABI 7, additive).  The pair chip_frame_put_orb_stereo takes is
 * the RECTIFIED one.  The reference receives the cameras' raw images and makes that pair on a host core, for both frames of every
 * candidate: StereoGeometry::do_stereo_rectification_of_raw_images (src/utils/CameraGeometry.cpp:387-402) is four
 * cv::remap(.., CV_INTER_LINEAR) per pair -- raw -> undistorted through the camera model's maps (:39-43, :361-372), undistorted ->
 * stereo-rectified through the cv::initUndistortRectifyMap maps of cv::stereoRectify (:348-349, :377-383) -- 4 w h bilinear gathers
 * through float maps.  The maps are calibration data: made once per calibration by camodocal / OpenCV code that stays on the host and
 * handed over once (chip_rectify_set_maps).  The raw pair is the same 2 w h bytes the rectified one is.
 *
 * THE DEFINITION IS THIS PROJECT'S OWN, all-integer after the quantiser, modelled on cv::remap with INTER_LINEAR, float maps and
 * BORDER_CONSTANT 0, restated in tests/np_mirror_rectify.py (which the device equals bit for bit).  OpenCV's source is not part of this
 * project, so parity against it is UNPINNED (DESIGN.md 6 lists the known departures).
 *   - quantiser: a map value m (float) becomes q = Q(m), an int32 in 1/32 pixel.  NaN gives -64; otherwise
 *       q = (int32) rint(32.0f * min(max(m, -2.0f), 32768.0f)),  rounding to nearest, ties to even
 *     (the product is exact in float; -0.0 gives 0; +-inf clamp; 3.015625 -> 96, 3.046875 -> 98).  A coordinate at or beyond a clamp
 *     has every tap outside any supported image, so no sentinel is needed.  x0 = q >> 5 (arithmetic shift), a = q & 31; the same in
 *     y gives y0 and b.  chip_rectify_quantize is Q on the host;
 *   - sample: with I[y][x] = 0 outside [0, h) x [0, w),
 *       S(I, qx, qy) = (I[y0][x0] (32-a)(32-b) + I[y0][x0+1] a (32-b) + I[y0+1][x0] (32-a) b + I[y0+1][x0+1] a b + 512) >> 10
 *     the exact bilinear value at 1/32-pixel resolution, rounded half up;
 *   - one stage:  R[y][x] = S(raw, q1x[y][x], q1y[y][x]);
 *   - two stages (the reference's shape):  U[y][x] = S(raw, q1x[y][x], q1y[y][x]), a uint8 as the undistorted image is in the
 *     reference, and  R[y][x] = S(U, q2x[y][x], q2y[y][x]).  All images and maps have one size w x h;
 *   - kernel rectify_pair: ONE launch for both eyes (a grid axis) and both stages.  U is never written: an output pixel reads its
 *     stage-2 entry and evaluates stage 1 at each of its four U taps that lies inside the image, from that tap's stage-1 entry and
 *     four raw bytes, rounded to uint8 before stage 2 weighs it -- a U pixel is a pure function of (raw, q1) at that pixel, so the
 *     result is bit for bit the two-pass one.  A thread makes four consecutive pixels of a row and stores them as one dword where the
 *     row's alignment allows.  The quantised maps lie interleaved (qx, qy) on the device; the header fixes only the arithmetic;
 *   - chip_remap: one stage with the caller's maps into host memory (the definition made callable, the same kernel on one image with
 *     a per-call map upload; not a hot path).  NULL ctx / image / map_x / map_y / out or a side < 1 CHIP_ERR_INVALID_ARG; a side
 *     beyond the image limit of chip_match_pair or a group ctx CHIP_ERR_UNSUPPORTED; all decided before the device is touched.
 *     Needs no frame store and no maps; runs on the ctx stream, serialised with the other calls of the stage;
 *   - chip_rectify_set_maps: quantises the maps on the host and uploads them once.  They replace any maps the ctx had (after a
 *     failure behind the argument checks the ctx has none) and are freed with the ctx.  The stage-1 maps of both eyes are required;
 *     the four stage-2 pointers are all non-NULL (two stages) or all NULL (one stage), a mix is CHIP_ERR_INVALID_ARG as are a NULL
 *     ctx and a side < 1; a side above CHIP_ORB_MAX_SIDE or a group ctx CHIP_ERR_UNSUPPORTED.  Needs no frame store; a process that
 *     never calls it allocates nothing.  With the reference's names the eight arguments are the left camera's map_x, map_y,
 *     map1_x, map1_y and the right camera's map_x, map_y, map2_x, map2_y;
 *   - chip_rectify_pair: the dense rectified pair into host memory through the ctx's maps, for callers that stay on host frames.
 *     NULLs or a side < 1 CHIP_ERR_INVALID_ARG, a group ctx CHIP_ERR_UNSUPPORTED, no maps set CHIP_ERR_BUSY, a size other than the
 *     maps' CHIP_ERR_INVALID_ARG;
 *   - chip_frame_put_raw_orb_stereo: chip_frame_put_orb_stereo with the raw pair in the place of the rectified one.  The raw pair is
 *     staged behind the place where chip_frame_put_orb_stereo stages its pair, rectify_pair writes the rectified pair there, and from
 *     there on the call IS the other one (one body).  Every rule, status and failure behaviour of chip_frame_put_orb_stereo holds,
 *     in its order; in addition, behind the CHIP_ERR_BUSY of a missing reserve, no maps set is CHIP_ERR_BUSY and a size other than
 *     the maps' CHIP_ERR_INVALID_ARG.  All statuses are decided before the device is touched; each image crosses the bus once; one
 *     count comes back.  The frame is indistinguishable from chip_rectify_pair -> chip_frame_put_orb_stereo.                       */
int chip_build_has_rectify(void);          /* 1 */
int chip_rectify_quantize(const float *map, int64_t count, int32_t *q /* count */);
int chip_remap(chip_ctx *ctx, const uint8_t *image /* height x width, dense rows */, int32_t width, int32_t height,
               const float *map_x, const float *map_y /* height x width each */, uint8_t *out /* height x width, host */);
int chip_rectify_set_maps(chip_ctx *ctx, int32_t width, int32_t height, const float *lx1, const float *ly1,
                          const float *lx2, const float *ly2 /* both NULL: one stage */, const float *rx1, const float *ry1,
                          const float *rx2, const float *ry2 /* as lx2, ly2 */);
int chip_rectify_pair(chip_ctx *ctx, const uint8_t *left_raw, const uint8_t *right_raw, int32_t width, int32_t height,
                      uint8_t *left_out, uint8_t *right_out /* height x width each, host */);
int chip_frame_put_raw_orb_stereo(chip_ctx *ctx, int64_t id, int32_t width, int32_t height, const uint8_t *left_raw,
                                  const uint8_t *right_raw, const chip_orb_params *orb /* NULL: the defaults */,
                                  const chip_stereo_bm_params *bm /* NULL: the defaults */, const double Q_rowmajor[16], int32_t *n);

/* ------------------------------------------------------------------------------------------ many pairs per call
 * Every other leg of the verification path takes a batch; these calls are the frame put's.  A restarted node, an offline replay and the
 * consumer thread's backlog put frames in bulk, and a single put is mostly launch chains and host waits (16 launches and two waits a
 * frame), with its longest kernel on eight workgroups.  A batched call walks its F pairs in GROUPS: every stage runs ONCE per group
 * over all its frames (the frame is a grid axis; the pyramid stays one launch per level), the detector writes each frame's descriptor
 * and keypoint rows straight into its slot, the block matcher reads each frame's kept count in device memory, and the host waits once
 * per group for the F x 8 counts of one copy.
 *   - shared inputs: width, height, both parameter blocks and Q hold for every frame of the call -- one rig, as the ctx's maps;
 *   - result: for every f the stored rows of ids[f] (what chip_frame_read returns) and n[f] are BYTE FOR BYTE what
 *     chip_frame_put_orb_stereo / chip_frame_put_raw_orb_stereo give for that pair (one body per kernel, two entries).  A frame
 *     without keypoints is stored with n = 0;
 *   - groups: as many frames as keep the group's level-0 pixels <= 2^23, at most 16, at least 1 (16 up to 724 x 724; 10 at
 *     1024 x 768; 1 at 4096 x 4096).  chip_frame_put_plan says so without a ctx (raw 0 / 1: which call; the plan is the same);
 *     chip_debug_frame_put_last reports the groups, kernel launches and host waits of the ctx's last batched call (every output may be
 *     NULL; zeros before the first).  A group is its uploads, at most 16 launches, one copy of counts and one wait;
 *   - checks, in this order, all before the first write: NULL ctx / ids / left / right / Q / n, F < 1, a NULL image or an id that
 *     repeats inside the call CHIP_ERR_INVALID_ARG;  F > CHIP_FRAME_MAX_PUT, a size or parameter chip_orb_detect or chip_stereo_bm
 *     refuses (a side < 1 is theirs: CHIP_ERR_INVALID_ARG), a group ctx, n_features > slot_keypoints CHIP_ERR_UNSUPPORTED;  no
 *     chip_frame_store_reserve yet, or no maps for the raw form CHIP_ERR_BUSY;  the raw form: a size other than the maps'
 *     CHIP_ERR_INVALID_ARG;  fewer free slots than ids of the call that are not yet stored CHIP_ERR_OOM -- the store is then exactly as
 *     it was (as it is after CHIP_ERR_OOM for scratch that could not grow, which is decided before the first group);
 *   - commit and failure: an id already stored is replaced in its own slot; new ids take free slots, which need not be adjacent.
 *     Groups commit as they finish.  A HIP error in group g keeps the frames of the groups before it, removes group g's ids from the
 *     store (a replaced id's rows are undefined by then) and leaves later groups untouched; n[f] of group g and of the later ones
 *     is -1;
 *   - memory: the scratch of a group (G x a single call's) is grown inside one pause of the resident scan; a process that never
 *     calls a batch form allocates nothing more than before.  After a batched call chip_debug_orb_level / _blur are CHIP_ERR_BUSY;
 *   - chip_frame_put_records: what chip_frame_read gave (desc, kp_xy, the point records) back into the store under id -- three
 *     uploads, no kernel; the statuses of chip_frame_put with pts in the place of the 3-D image.  The fourth float of a record must
 *     be the 0.0f (no point) or 1.0f the gather kernels write, bit for bit: anything else is CHIP_ERR_INVALID_ARG, decided on the
 *     host before the store is touched.  A frame put this way is indistinguishable afterwards: a checkpoint of records restores a
 *     store without the images.                                                                                                     */
#define CHIP_FRAME_MAX_PUT 256
int chip_build_has_frame_put_batch(void);  /* 1 */
int chip_frame_put_plan(int32_t width, int32_t height, const chip_orb_params *orb /* NULL: the defaults */, int32_t raw, int32_t F,
                        int32_t *group /* frames per group */, int32_t *n_groups);
int chip_frame_put_orb_stereo_batch(chip_ctx *ctx, const int64_t *ids, int32_t F, int32_t width, int32_t height,
                                    const uint8_t *const *left, const uint8_t *const *right /* F images each */,
                                    const chip_orb_params *orb /* NULL: the defaults */,
                                    const chip_stereo_bm_params *bm /* NULL: the defaults */, const double Q_rowmajor[16],
                                    int32_t *n /* F */);
int chip_frame_put_raw_orb_stereo_batch(chip_ctx *ctx, const int64_t *ids, int32_t F, int32_t width, int32_t height,
                                        const uint8_t *const *left_raw, const uint8_t *const *right_raw /* F images each */,
                                        const chip_orb_params *orb /* NULL: the defaults */,
                                        const chip_stereo_bm_params *bm /* NULL: the defaults */, const double Q_rowmajor[16],
                                        int32_t *n /* F */);
int chip_frame_put_records(chip_ctx *ctx, int64_t id, const uint8_t *desc /* n x 32 */, const float *kp_xy /* n x 2 */,
                           const float *pts /* n x 4 */, int32_t n, int32_t width, int32_t height);
int chip_debug_frame_put_last(chip_ctx *ctx, int32_t *groups, int32_t *launches, int32_t *waits);

/* ------------------------------------------------------------------------------------------ introspection */
typedef struct {
    int32_t abi_version;
    int32_t D;
    int32_t device;
    int32_t shard_rank, shard_count;
    int32_t n_cus;              /* multiProcessorCount                                             */
    int64_t rows_global;        /* == chip_db_size                                                 */
    int64_t rows_local;         /* rows stored on this rank                                        */
    int64_t capacity_local;     /* rows reserved on this rank                                      */
    int64_t lossy_rows;         /* rows appended with CHIP_APPEND_ALLOW_ROUNDING that actually rounded */
    char    arch[32];           /* gcnArchName, e.g. "gfx950:sramecc+:xnack-"                      */
    int32_t storage_bytes;      /* 4 = float rows, 8 = double rows                                 */
    int32_t n_devices;          /* 1, or G of chip_create_multi (then the other fields describe devices[0]) */
    int32_t exchange;           /* CHIP_EXCHANGE_*                                                 */
    int32_t comm_ranks;         /* ranks of the RCCL communicator the exchange runs over (ncclCommCount), 0 = none: a caller
                                   that asked for G GPUs can PROVE the collective spans G ranks (and see a copy fallback) */
    int32_t comm_init_abandoned;/* 1: an RCCL bootstrap of this ctx (ncclCommInitAll in chip_create_multi, ncclCommInitRank in
                                   chip_comm_init_rank) did not return within CHIP_COMM_INIT_TIMEOUT_MS (default 120 s) and was
                                   abandoned on its helper thread; the ctx works (a group: over the copy exchange), but process
                                   teardown may block inside RCCL -- leave through _exit() once the work is done (ABI 4)      */
    int32_t scan_forms;         /* CHIP_SCAN_FORM_* bits: which forms of the scan kernel this build of the library contains (ABI 5).
                                   The row-batched form (short prefixes) depends on how the building hipcc allocates registers; a
                                   build whose code-object check failed is made with -DCHIP_NO_ROWS_FORM and serves every scan with
                                   the one-row kernel -- same results, short prefixes slower                                    */
    int32_t test_hooks;         /* 0: the product build (`make lib`): no fault-injection hook, no test knob is compiled in, the
                                   CHIP_TEST_* / CHIP_PNP_BACKSUB / CHIP_PNP_DEBUG_STOP environment variables are never read.
                                   1: the test build (-DCHIP_TEST_HOOKS, `make testlibs` -> cerebro_amd/lib/hooks/), which only
                                   tests/ load -- never deploy it (ABI 6)                                                       */
    double  row_norm_max;       /* float rows: an upper bound on the L2 norm of every published row (the largest fp64 row norm, times
                                   1 + 2^-30); 0 for an empty DB and for double rows.  The prefilter pass takes its error bound from it
                                   (ABI 7, additive: the last field)                                                              */
} chip_info;
enum { CHIP_SCAN_FORM_ONE_ROW = 1, CHIP_SCAN_FORM_ROWS = 2 };
/* the same bits without a ctx (what `make verify` and the build log ask) */
int chip_build_scan_forms(void);
/* chip_info.test_hooks without a ctx */
int chip_build_test_hooks(void);
enum { CHIP_EXCHANGE_NONE = 0, CHIP_EXCHANGE_RCCL = 1, CHIP_EXCHANGE_COPY = 2 };
int chip_get_info(const chip_ctx *ctx, chip_info *info);

/* Per-kernel timing on the ctx stream (hipEvents bracketing every scan launch). */
int chip_profile_enable(chip_ctx *ctx, int32_t on);
int chip_profile_reset(chip_ctx *ctx);
/* Sum of the per-launch durations (ms) and launch count of the dominant kernel (db_scan_topk) since reset, plus the
 * busy span first-start -> last-stop; total_ms / span_ms (the
 * measured concurrency) stays ~1: scans are serialised on one internal stream. */
int chip_profile_scan(chip_ctx *ctx, double *total_ms, int64_t *n_launches, double *bytes_per_launch_last, double *span_ms);

#ifdef __cplusplus
}
#endif
#endif
