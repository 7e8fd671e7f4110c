/*
 * wfsparse.h -- C ABI of libwfsparse.so: the MI355X (gfx950) sparse-convolution hot path of
 * WaveformML's LitPSD training step.
 *
 * This is the drop-in boundary.  Every entry point replaces one operator of the third-party
 * package the reference calls for this path, spconv~=1.2.1 (reference requirements.txt:15), i.e.
 * the torch custom ops behind its Python surface:
 *
 *   torch.ops.spconv.get_indice_pairs      <- spconv.ops.get_indice_pairs, called from
 *       SparseConvolution.forward for every layer the reference constructs at
 *       src/models/SPConvBlocks.py:75,134,191,249,298,335,370,498,502,803,809 and by config
 *       strings "spconv.SubMConv3d" etc. (src/utils/ModelValidation.py:24-31)
 *   torch.ops.spconv.indice_conv           <- spconv.functional.indice_conv / indice_subm_conv /
 *   torch.ops.spconv.indice_conv_backward     indice_inverse_conv (same call sites; inverse conv
 *                                             at src/models/SPConvBlocks.py:804,810)
 *   SparseConvTensor.dense()               <- spconv.ToDense (src/models/SPConvBlocks.py:81,515),
 *                                             src/engineering/LitBase.py:138-146
 *
 * Conventions
 *   - plain C types only: raw DEVICE pointers (HBM), sizes, and an opaque hipStream_t passed as
 *     void*.  No torch types.  The library owns no memory and keeps no global state besides a
 *     thread-local error string and an opt-in event-timing table; all outputs and workspaces
 *     are caller-allocated (two-phase "plan" -> "run" where a size is data dependent).
 *   - every call is asynchronous on `stream` unless documented otherwise.
 *   - return value: 0 = WFS_OK, otherwise one of WFS_E*; wfs_last_error() gives the text.
 *     The Python shim maps WFS_EINVAL -> AssertionError / RuntimeError as spconv raises them
 *     (SURVEY.md 8b "Error conventions").
 *   - index tensors are int32, batch-first [N, ndim+1] exactly as spconv's (the reference
 *     permutes its (x,y[,t],evt) columns to batch-first at src/models/SPConvNet.py:47-52,64).
 *   - feature dtype codes: WFS_F32 (fp32 storage, fp32 accumulate), WFS_BF16 and WFS_F16 (16-bit
 *     storage, fp32 accumulate; the reference's `half_precision` rows are fp16,
 *     src/datasets/HDF5Dataset.py:227).  Filters [K, Cin, Cout] are fp32 in every case (master
 *     weights, rounded to the storage type while they are staged for the matrix cores).
 *   - device-side row counts: every row-dimensioned call takes its row count BY VALUE (array
 *     strides, grid size, = the capacity) and an optional `const int64_t *..._dev` that, when not
 *     NULL, holds the number of VALID rows (<= the capacity) in device memory.  Rows beyond it are
 *     neither read nor written.  With device counts no call needs the host to know a data-dependent
 *     size, so a whole training step can be captured into one HIP graph and replayed.
 */
#ifndef WFSPARSE_H
#define WFSPARSE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WFS_OK 0
#define WFS_EINVAL 1      /* bad argument / unsupported configuration                    */
#define WFS_EOVERFLOW 2   /* batch * prod(out_shape) >= 2^31 (spconv asserts the same)    */
#define WFS_EHIP 3        /* a HIP runtime call failed                                    */
#define WFS_EWORKSPACE 4  /* workspace too small                                          */

#define WFS_F32 0
#define WFS_BF16 1
#define WFS_F16 2

#define WFS_MAX_DIM 4

/* library / device ------------------------------------------------------------------------
 * WFS_ABI_VERSION changes whenever a struct layout, an exported signature or the meaning of an argument does (3: wfs_geometry grew
 * `transposed` / `output_padding` in round 2, the event-local build joined in round 3; 4: the wide-layer entry points; 5: the failure flags of wfs_rulebook_emit and
 * wfs_event_rulebook_subm are sticky -- set, never cleared, by the library; 6: round 4 -- wfs_gather_conv / wfs_gather_dw take
 * `packed_kl`, the event-local build of regular convolutions and the packed by-input table joined).  A binding
 * compiled against another version must refuse the library: waveformml_amd/_lib.py does. */
#define WFS_ABI_VERSION 6
int wfs_abi_version(void);
const char *wfs_last_error(void);

/* Geometry of one sparse convolution, host side (all arrays have ndim entries).
 * For SubM the front door forces stride = 1, padding = ksize/2, out_shape = spatial
 * (SURVEY.md A.2); call wfs_geometry_init to apply those rules and validate.              */
typedef struct wfs_geometry {
    int32_t ndim;
    int32_t batch_size;
    int32_t subm;
    int32_t K;                          /* prod(ksize), filled by wfs_geometry_init          */
    int32_t spatial[WFS_MAX_DIM];       /* input spatial shape                               */
    int32_t out_shape[WFS_MAX_DIM];     /* filled by wfs_geometry_init                       */
    int32_t ksize[WFS_MAX_DIM];
    int32_t stride[WFS_MAX_DIM];
    int32_t padding[WFS_MAX_DIM];
    int32_t dilation[WFS_MAX_DIM];
    int32_t transposed;                 /* != 0: spconv's SparseConvTranspose geometry (subm must be 0)   */
    int32_t output_padding[WFS_MAX_DIM];/* transposed only                                                  */
} wfs_geometry;

/* Validates and completes a geometry (replaces the Python front door of
 * spconv.ops.get_indice_pairs, A.2).  WFS_EINVAL if a dim has stride>1 and dilation>1,
 * WFS_EOVERFLOW if batch*prod(out_shape) >= 2^31.
 * transposed != 0 (spconv.SparseConvTranspose{2,3}d -- named by the reference at src/utils/ModelValidation.py:30-31):
 * out_shape = (i - 1) s - 2 p + k + output_padding (spconv's get_deconv_output_size: dilation does not enter), input
 * (x, offset o) reaches output x s - p + o d, outputs numbered first-seen with the offsets of a row visited from the
 * LAST to the first (getValidOutPosTranspose walks from the upper corner down).  PARITY UNPINNED on that order: the
 * spconv source is not available here and the reference never constructs one; values are pinned by dense
 * torch conv_transpose (tests).                                                                                       */
int wfs_geometry_init(wfs_geometry *g);

/* rulebook ---------------------------------------------------------------------------------
 * Replaces torch.ops.spconv.get_indice_pairs.  Besides spconv's own encoding
 * (indice_pairs int32 [2,K,N] padded with -1, indice_pair_num int32 [K], both bit-identical
 * to the CPU algorithm of A.3, including first-seen output numbering) the build produces the
 * gather tables the compute kernels consume:
 *     nbr_out int32 [K, N] : for input row j and kernel offset k, the output row, or -1
 *     nbr_in  int32 [K, M] : for output row i and kernel offset k, the input row, or -1
 * (SubM with odd kernels and dilation 1: nbr_in[k] == nbr_out[K-1-k], so nbr_in may be NULL.)
 *
 * Phase 1  wfs_rulebook_plan : site table build (hash or direct grid), candidate lookup,
 *          first-seen numbering.  SubM: nbr_out is final.  Regular conv: nbr_out holds table
 *          slots until phase 2.  Synchronises `stream` ONCE to return, on the host,
 *          host_info = {M, input_has_duplicate_coordinates (SubM only)}.  For SubM host_info may
 *          be NULL: no read-back, no synchronisation -- the caller then vouches that every index
 *          row is in range and that sites are distinct (spconv itself checks neither).
 * Phase 2  wfs_rulebook_emit : regular conv: writes out_indices [M, ndim+1], finalises nbr_out,
 *          fills nbr_in [K, M] if given.  SubM: fills nbr_in if given (needed only for even
 *          kernels / dilation).  Both: spconv's indice_pairs / indice_pair_num if given
 *          (indice_pair_num alone is allowed; pass NULL for both to skip the compaction).
 *
 * `workspace` must hold wfs_rulebook_workspace_bytes(g, N) bytes and stay untouched between
 * the two phases.  WFS_EINVAL if an index row lies outside batch_size / spatial.
 *
 * Device-count mode (no host synchronisation at all): host_info = NULL, n_dev = valid input rows,
 * m_dev = where the plan writes min(M, M_cap) for the consumers of the outputs, M_cap = the caller's
 * output capacity (rows of out_indices / nbr_in handed to emit as M); emit sets *overflow_dev = 1
 * if the true M exceeded it (the step's results are then invalid and must be redone with room) and
 * leaves it alone otherwise: the flag is STICKY, the caller clears it before the first build and
 * after reading it (a captured step replays many builds between two reads). */
size_t wfs_rulebook_workspace_bytes(const wfs_geometry *g, int64_t N);

int wfs_rulebook_plan(const wfs_geometry *g, const int32_t *indices, int64_t N,
                      int32_t *nbr_out, void *workspace, size_t workspace_bytes,
                      int64_t host_info[2], const int64_t *n_dev, int64_t *m_dev, int64_t M_cap,
                      void *stream);

int wfs_rulebook_emit(const wfs_geometry *g, const int32_t *indices, int64_t N, int64_t M,
                      int32_t *nbr_out, int32_t *out_indices, int32_t *nbr_in,
                      int32_t *indice_pairs, int32_t *indice_pair_num,
                      void *workspace, size_t workspace_bytes, const int64_t *n_dev,
                      int32_t *overflow_dev, void *stream);

/* Duplicate-coordinate / range check of an index set whose uniqueness is unknown before a
 * REGULAR conv (SubM learns it for free in its plan; a regular conv's output is unique by
 * construction).  g_subm: a SubM geometry over the set's own spatial shape; workspace as for
 * that geometry.  Synchronises.  host_info = {N, has_duplicates}.                           */
int wfs_indices_check(const wfs_geometry *g_subm, const int32_t *indices, int64_t N,
                      void *workspace, size_t workspace_bytes, int64_t host_info[2], void *stream);

/* gather - GEMM - (no) scatter --------------------------------------------------------------
 * Replaces torch.ops.spconv.indice_conv (forward) and the dX half of indice_conv_backward.
 * Output-stationary: every output row r gathers its <= K source rows through
 * table [K, R] (entry -1 = no neighbour) and contracts them with the per-offset filter:
 *     Y[r, :] = bias + sum_k  X[table[kmap[k], r], :] . W[k]            (transpose_w == 0)
 *     Y[r, :] =        sum_k  X[table[kmap[k], r], :] . W[k]^T          (transpose_w == 1)
 * W is fp32 [K, Cw_in, Cw_out]; with transpose_w the contraction runs over Cw_out.
 * kmap (host array of K ints, may be NULL = identity) lets SubM reuse nbr_out as nbr_in.
 * identity_k >= 0 names the offset whose source row is r itself (SubM centre: spconv computes
 * it as a plain X.W[k*] with k* = argmax indice_pair_num, A.4); -1 = none.  table may be NULL
 * only for K == 1 && identity_k == 0.
 * No atomics: each output row is written exactly once, results are run-to-run reproducible.
 * Packed tables (round 4).  Where a regular conv's kernel is no longer than its stride along the LAST dimension
 * (the PSD nets' SparseConv3d k 3, stride (1,1,4): reference src/models/SPConvBlocks.py:498 through config strings) an
 * input row reaches at most ONE output cell per leading kernel offset q, so the by-input table of
 * wfs_event_rulebook_conv is [K / kl, R] instead of [K, R]: entry e >= 0 means "row e >> 3, at kernel offset
 * k = q * kl + (e & 7)", -1 = none (9 instead of 27 table rows at that geometry, 54 % instead of 18 % of them used).
 * packed_kl = kl hands such a table to wfs_gather_conv (transpose_w products, i.e. dX) and wfs_gather_dw; 0 = the
 * dense form.  wfs_gather_packed_ok(kl, K, Ca, Cb, dtype, which) tells whether a product takes it (which = 1: dX,
 * 2: forward, 3: dW); wfs_unpack_table expands a packed table to the dense one for every other consumer.
 * Arithmetic of fp32 rows (WFS_F32), 32 -> 32 channels (round 4): every fp32 number -- rows and filters -- is cut into
 * three bf16 pieces whose sum is the number exactly, and the six leading piece products are summed in fp32 on
 * v_mfma_f32_16x16x32_bf16 / _32x32x16_bf16 (csrc/conv_mfma.hip k_gconv16_split, k_gdw32_split); what is left out is
 * below 2^-24 of the leading product, the size of one fp32 rounding -- the same 1e-5 bar as the fp32 instructions
 * (v_mfma_f32_16x16x4_f32, taken with the environment's WFS_SPLIT_BF16=0) at 0.6x their time.  Non-finite inputs give
 * NaN (Inf - Inf inside the cut) where an fp32 product would give +-Inf. */
int wfs_gather_conv(const int32_t *table, const int32_t *kmap_host, int32_t K, int32_t identity_k,
                    int64_t R, const void *X, int64_t X_rows, int32_t Cx, const float *W,
                    int32_t Cw_in, int32_t Cw_out, int32_t transpose_w, const float *bias, void *Y,
                    int32_t dtype, const int64_t *r_dev, int32_t packed_kl, void *stream);
int wfs_gather_packed_ok(int32_t packed_kl, int32_t K, int32_t Ca, int32_t Cb, int32_t dtype, int32_t which);
int wfs_unpack_table(const int32_t *packed, int32_t K, int32_t packed_kl, int64_t R, const int64_t *r_dev,
                     int32_t *dense, void *stream);

/* Wide layers as dense matrix-core products (round 3; csrc/wide.hip).
 * Same contract as wfs_gather_conv -- replaces torch.ops.spconv.indice_conv / the dX half of
 * indice_conv_backward (spconv 1.2.1 ops.py; the reference reaches them from src/models/SPConvBlocks.py:450-516
 * with 1697 / 1021 / 345 channels, BASELINE configs[4]) and, with K == 1 && table == NULL, the torch.mm of a
 * 1 x 1 SparseConv2d (spconv conv.py: `features = torch.mm(input.features, weight.view(in, out))`) -- when a side
 * of the filter has >= 128 channels: the layer runs as ONE dense product over whichever side (X_rows source rows,
 * R destination rows) is shorter, on v_mfma_f32_32x32x16_{bf16,f16} for 16-bit rows (filters rounded to the row
 * type) and on v_mfma_f32_32x32x2_f32 for fp32 rows (an exact fp32 fma chain: the 1e-5 path), fp32 accumulate,
 * ordered fp32 sum over the kernel offsets, every output row written once (no atomics).
 * wfs_wide_conv_ok: does this path take the shape?  The workspace holds the filters in the row type, the padded /
 * gathered rows and the per-offset products; 16-byte aligned. */
int wfs_wide_conv_ok(int32_t K, int64_t R, int64_t X_rows, int32_t Cx, int32_t Cy, int32_t dtype);
/* A/B switch for benchmarks (tools/microbench_generic.py): 0 sends every layer back to the 32 x 32-tile kernels
 * (wfs_gather_conv / the narrow arm of wfs_gather_dw); a value >= 8 turns the path on for layers with at least that
 * many channels on a side.  Returns the previous threshold (0 = was off). */
int wfs_wide_enable(int32_t on);
size_t wfs_wide_conv_workspace_bytes(int32_t K, int64_t R, int64_t X_rows, int32_t Cx, int32_t Cy,
                                     int32_t has_table, int32_t dtype);
/* The filters as the products read them: [K][Cw_in][Cw_out rounded up to whole 16-byte pieces] in the row type,
 * zero padded.  A caller that runs several products on the same filters (the forward pass and dX of one layer)
 * converts them once (wfs_wide_filters) and hands the copy to wfs_wide_gather_conv as Wp; with Wp == NULL every
 * call converts W into its workspace (fp32 filters whose rows are whole pieces are read in place). */
size_t wfs_wide_filters_bytes(int32_t K, int32_t Cw_in, int32_t Cw_out, int32_t dtype);
int wfs_wide_filters(const float *W, int32_t K, int32_t Cw_in, int32_t Cw_out, int32_t dtype, void *Wp,
                     void *stream);
int wfs_wide_gather_conv(const int32_t *table, const int32_t *kmap_host, int32_t K, int32_t identity_k,
                         int64_t R, const void *X, int64_t X_rows, int32_t Cx, const float *W, const void *Wp,
                         int32_t Cw_in, int32_t Cw_out, int32_t transpose_w, const float *bias, void *Y,
                         int32_t dtype, const int64_t *r_dev, void *workspace, size_t workspace_bytes,
                         void *stream);
/* Rows at or beyond *r_dev of wfs_wide_gather_conv's Y are not written, whichever product order the layer takes
 * (the direct store of the product and the ordered sum both take the count). */

/* What a wide product of a shape would launch, host only, nothing launched (tests/test_wide_cases_host.py reads from
 * it which arm a case runs; decided by the planning helpers of csrc/wide.hip themselves).  kind 0: conv forward / dX
 * (K, R, X_rows, Ca = Cx, Cb = Cy with the channel roles as wfs_wide_gather_conv's caller swaps them, has_table);
 * 1: conv dW (K, R, Ca = Cs, Cb = Cg); 2: linear forward and 3: linear dW (R = B, Ca = I, Cb = O).  out[7] (may be
 * NULL): dense_first, nz, nseg, ksplit, kchunk, the fp32 slabs the ordered sum adds per output element (0: it does
 * not run), the slabs of one offset among them.  Returns 1 / 0 = the wide path takes / does not take the shape
 * (wfs_wide_conv_ok, the dW arm of wfs_gather_dw, wfs_wide_linear_ok), -WFS_EINVAL for refused arguments.
 * Additions only: WFS_ABI_VERSION stays. */
int wfs_wide_plan(int32_t kind, int32_t K, int64_t R, int64_t X_rows, int32_t Ca, int32_t Cb, int32_t has_table,
                  int32_t dtype, int32_t *out);

/* Dense head layer on the matrix cores (round 3; csrc/wide.hip).
 * Replaces torch.nn.functional.linear for the reference's dense head when it is wide (the hybrid net's
 * Linear(24150, 269), src/models/SPConvNet.py:40-52 through LinearBlock): y = x W^T + b with x [B, I] in the row
 * type, fp32 W [O, I] (nn.Linear's layout; rounded to the row type for a 16-bit product), fp32 accumulate, fp32 y.
 * The backward takes fp32 dY (rounded to the row type as an operand) and returns dX in the row type, dW / db in
 * fp32; any of the three may be NULL.  Contractions with few output tiles are cut into parts and summed in a fixed
 * order.  wfs_wide_linear_ok: I >= 256, O >= 9 (narrower heads: wfs_head_fwd). */
int wfs_wide_linear_ok(int64_t B, int32_t I, int32_t O, int32_t dtype);
size_t wfs_wide_linear_workspace_bytes(int64_t B, int32_t I, int32_t O, int32_t dtype);
int wfs_wide_linear_fwd(const void *X, int64_t B, int32_t I, const float *W, const float *bias, int32_t O, float *Y,
                        int32_t dtype, void *workspace, size_t workspace_bytes, void *stream);
int wfs_wide_linear_bwd(const void *X, const float *dY, int64_t B, int32_t I, const float *W, int32_t O, void *dX,
                        float *dW, float *db, int32_t dtype, void *workspace, size_t workspace_bytes, void *stream);

/* Event-local rulebook build (round 3; csrc/evrulebook.hip).
 * A sparse convolution never crosses events (the rulebook key includes the batch index) and the
 * reference's collate_fn concatenates the items of a batch in order (src/engineering/PSDDataModule.py:10-20), so the
 * rows of one event are one contiguous range of the index set.
 * wfs_event_offsets: indices int32 [N, ndim + 1] batch-first (n_dev as everywhere) -> offsets int32
 *   [wfs_event_offsets_ints(batch_size)] = { first row of event 0 .. batch_size - 1, number of valid rows,
 *   WFS_EVENT_FLAG_WORDS flag words }; a flag word != 0 <=> the batch column is NOT non-decreasing / in range.  Verified
 *   on the device by every launch; every word is written by every launch; nothing is read back.
 * wfs_event_rulebook_subm: torch.ops.spconv.get_indice_pairs(subm=True) for an index set grouped by event, ONE
 *   WORKGROUP PAIR PER EVENT with the event's site table in LDS (cell -> sample array, direct addressing) -- no site
 *   grid over the batch in HBM, no clearing launch, no global atomics: HBM traffic = the coordinates in, the table out.
 *   nbr_out is bit-identical to wfs_rulebook_plan's.  `events` = wfs_event_offsets of `indices`.
 *   flags: int32 [wfs_event_rulebook_flag_ints(batch)] = 3 x blocks words, STICKY: a launch sets words and never
 *   clears one -- the caller zeroes them before the first build and after reading them (a captured step replays many
 *   builds between two reads).  Any word != 0 in [0, blocks): the index set is not grouped by event or an event exceeds the LDS tables (64 KiB of
 *   sample arrays: 128 active cells at 256 samples) -- nbr_out is then incomplete and the caller takes wfs_rulebook_plan instead;
 *   in [blocks, 2 blocks): duplicate coordinates (same remedy: "the last row wins" is resolved by the chip-wide build);
 *   in [2 blocks, 3 blocks): an index outside the spatial shape.
 *   slots (may be NULL): 64-byte records per row, 32 uint16 slots = 1 + neighbour's row within the event, 0 = none (the
 *   operand form of the event-local conv experiment, tools/exp/event_local/).                                       */
#define WFS_EVENT_FLAG_WORDS 64
size_t wfs_event_offsets_ints(int32_t batch_size);
int wfs_event_offsets(const int32_t *indices, int64_t N, int32_t ndim, int32_t batch_size, const int64_t *n_dev,
                      int32_t *offsets, void *stream);
int wfs_event_rulebook_ok(const wfs_geometry *g);
size_t wfs_event_rulebook_flag_ints(int32_t batch_size);
int wfs_event_rulebook_subm(const wfs_geometry *g, const int32_t *indices, int64_t N, const int64_t *n_dev,
                            const int32_t *events, int32_t *nbr_out, void *slots, int32_t *flags, void *stream);

/* Event-local build of REGULAR (strided) convolutions, ONE launch (round 4; csrc/evconv.hip).
 * torch.ops.spconv.get_indice_pairs(subm=False) -- the reference's SparseConv3d / SparseConv2d layers,
 * src/models/SPConvBlocks.py:75,498 -- for an index set grouped by event, in device-count mode: one workgroup per event
 * keeps the event's OUTPUT grid in LDS (wfs_event_rulebook_conv_ok: <= 16384 cells per event, K <= 32, leading kernel
 * dims <= 4, not transposed), takes first-seen tickets with LDS atomics, numbers the event's sites by a block scan over
 * its rows and learns the ids of the events in front from per-event counts published in `state` (a single pass: no
 * site grid in HBM, no clearing launch, no global read-modify-write, every table written once).  Results are
 * bit-identical to wfs_rulebook_plan + wfs_rulebook_emit (oracle/spconv_ref.c:208-276).
 *   events_in   wfs_event_offsets table of `indices` (or the events_out of the conv that produced them)
 *   M_cap       rows of out_indices / stride of nbr_in; *m_dev = min(M, M_cap); *overflow_dev = 1 (sticky) if M > M_cap
 *   events_out  int32 [wfs_event_offsets_ints(batch)]: the same table for the OUTPUT rows (first-seen numbering of an
 *               event-grouped input is event-grouped)
 *   nbr_out     by-input table: packed_kl == 0: [K, N]; packed_kl == wfs_event_rulebook_conv_packed_kl(g) > 0:
 *               [K / kl, N] packed (see wfs_gather_conv)
 *   nbr_in      by-output table [K, M_cap] (may be NULL)
 *   cell_row    (may be NULL) int32 [batch * out_volume]: output row of every cell or -1 -- what wfs_to_dense_mapped
 *               takes as both `ticket` and `slot_id`
 *   flags       int32 [3], STICKY (set, never cleared): [0] the index set is not grouped by event, or a workgroup
 *               gave up waiting for a count (then *m_dev = 0 / tables invalid: take wfs_rulebook_plan), [2] an index
 *               outside the spatial shape (that row has no outputs)
 *   state       wfs_event_rulebook_conv_state_bytes(batch) bytes, 8-byte aligned, ZEROED once by the caller and then
 *               owned by this layer's builds (launch epoch + per-event counts); two builds must not run concurrently
 *               on one state. */
int wfs_event_rulebook_conv_ok(const wfs_geometry *g);
int wfs_event_rulebook_conv_packed_kl(const wfs_geometry *g);
size_t wfs_event_rulebook_conv_state_bytes(int32_t batch_size);
int wfs_event_rulebook_conv(const wfs_geometry *g, const int32_t *indices, int64_t N, const int64_t *n_dev,
                            const int32_t *events_in, int64_t M_cap, int32_t *out_indices, int64_t *m_dev,
                            int32_t *events_out, int32_t *nbr_out, int32_t packed_kl, int32_t *nbr_in,
                            int32_t *cell_row, int32_t *overflow_dev, int32_t *flags, void *state, void *stream);

/* Replaces the dW half of torch.ops.spconv.indice_conv_backward:
 *     dW[k, a, b] = sum_r  S[r, a] * G[table[k, r], b]          (swap == 0)
 *     dW[k, b, a] = sum_r  S[r, a] * G[table[k, r], b]          (swap == 1)
 * S = the stationary rows [R, Cs], G = the gathered rows [*, Cg]; table column kmap[k] serves
 * offset k (kmap_host NULL = identity; the SubM mirror is accepted for Cs = 32, Cg = 2, which lets
 * the first layer keep its wide dY rows stationary).  Deterministic two-stage reduction through
 * `workspace` (wfs_gather_dw_workspace_bytes).                                                 */
size_t wfs_gather_dw_workspace_bytes(int32_t K, int64_t R, int32_t Cs, int32_t Cg);

/* A pending second stage of wfs_gather_dw: dW = sum over `nslabs` partial results in `part` (the workspace).
 * With `defer` given, wfs_gather_dw runs only its first stage when the shape has a two-stage kernel and describes
 * the rest here (nslabs > 0; dW is NOT written yet, the workspace must stay alive); the caller later reduces the jobs
 * of a whole backward pass in ONE launch with wfs_dw_reduce_jobs -- at the PSD batch sizes every launch costs more
 * than the few hundred KB it reduces.  nslabs == 0 on return: nothing pending, dW is final. */
typedef struct wfs_dw_job {
    const float *part;
    int64_t nslabs;
    int64_t per;          /* elements of one slab = K * Cs * Cg */
    int32_t K, A, B;      /* slab layout [K][A][B] */
    int32_t transpose;    /* dW[k][b][a] = sum part[.][k][a][b] instead of dW[k][a][b] */
    float *dW;
} wfs_dw_job;

int wfs_gather_dw(const int32_t *table, const int32_t *kmap_host, int32_t K, int32_t identity_k,
                  int64_t R, const void *S, int32_t Cs, const void *G, int64_t G_rows, int32_t Cg,
                  int32_t swap, float *dW, int32_t dtype, void *workspace, size_t workspace_bytes,
                  const int64_t *r_dev, wfs_dw_job *defer, int32_t packed_kl, void *stream);

/* torch.ops.spconv.indice_conv_backward as ONE call (round 4): dW[k] = X^T . dY[table[k]] (as wfs_gather_dw with
 * swap == 0) and dX = sum_k dY[table[k]] . W[k]^T (as wfs_gather_conv with transpose_w), both through the by-input
 * table of a conv / SubM layer (dense [K, R] or packed, packed_kl as above).  X [R, Cin] = the layer's input rows, dY
 * [dY_rows, Cout], W fp32 [K, Cin, Cout], dX [R, Cin], dW fp32 [K, Cin, Cout].  For 32 -> 32 layers with 16-bit rows
 * both products run in ONE launch (independent blocks of one grid: the second product no longer waits for the first
 * one's last block, and a kernel boundary of ~4.6 us inside a captured step goes); other shapes run the two entry
 * points one after the other.  Results are bit-identical to the separate calls.  workspace / defer as wfs_gather_dw. */
int wfs_conv_backward(const int32_t *table, int32_t K, int32_t identity_k, int64_t R, const void *X, const void *dY,
                      int64_t dY_rows, int32_t Cin, int32_t Cout, const float *W, void *dX, float *dW, int32_t dtype,
                      void *workspace, size_t workspace_bytes, const int64_t *r_dev, wfs_dw_job *defer,
                      int32_t packed_kl, void *stream);

/* Second stage of up to 16 deferred wfs_gather_dw calls in one launch (deterministic: fixed summation order). */
int wfs_dw_reduce_jobs(const wfs_dw_job *jobs, int32_t n, void *stream);

/* Backward of  y = [relu](BatchNorm(z)),  z = first conv (2 -> 32 channels, no bias, K <= 27) of the network input X,
 * in training mode (batch statistics), for 16-bit rows: dW [K, 2, 32], dgamma and dbeta as wfs_bn_relu_bwd followed by
 * wfs_gather_dw (swap == 1) compute them -- the same arithmetic, roundings and summation orders, hence the same bits --
 * in two launches instead of three and without the [R, 32] dz tensor.  The first layer has no dX, so dz is needed only
 * as the stationary operand of the dW product: after the BatchNorm backward's reduce launch one kernel folds the
 * partial sums, forms dz = gamma * invstd * (g - sum g / N - xhat * sum g xhat / N) per tile in registers, rounds it
 * to the row type and contracts it with the gathered input rows.
 * table / kmap_host / identity_k / R / r_dev: the by-output table as wfs_gather_dw takes it for this layer (kmap NULL,
 * the identity or the SubM mirror).  Z, dY [R, 32] and X [X_rows, 2] have `dtype` WFS_BF16 or WFS_F16; dgamma / dbeta
 * may be NULL.  `defer` as in wfs_gather_dw (an ordinary job: the slabs hold dW partials); dgamma and dbeta are written
 * by the call itself either way.  Deterministic, no atomics.  Additions only: WFS_ABI_VERSION stays. */
size_t wfs_first_conv_bn_backward_workspace_bytes(int32_t K, int64_t R);
int wfs_first_conv_bn_backward(const int32_t *table, const int32_t *kmap_host, int32_t K, int32_t identity_k, int64_t R,
                               const void *Z, const void *dY, const void *X, int64_t X_rows, const float *gamma,
                               const float *beta, const float *save_mean, const float *save_invstd, int32_t relu,
                               float *dW, float *dgamma, float *dbeta, int32_t dtype, void *workspace,
                               size_t workspace_bytes, const int64_t *r_dev, wfs_dw_job *defer, void *stream);

/* Conv bias gradient: out[c] = sum over the valid rows of X[r][c] (fp32 sums of fp32 / bf16 / fp16 rows; r_dev as
 * everywhere: NULL = R exact, else R is the capacity).  What autograd computes for spconv's `out_features += bias`
 * (reference layers with trainable_weights=True, src/models/SPConvBlocks.py:498).  Deterministic (fixed orders).      */
size_t wfs_column_sum_workspace_bytes(int32_t C);
int wfs_column_sum(const void *X, int64_t R, int32_t C, float *out, void *workspace, size_t workspace_bytes,
                   int32_t dtype, const int64_t *r_dev, void *stream);

/* Scatter form with fp32 atomics, used ONLY when the input holds duplicate coordinates (then
 * the inverse of a gather table is not a function):
 *     Y_accum[table[k, r], :] += X[r, :] . W[k]  (or W[k]^T)      Y_accum fp32, caller-initialised */
int wfs_scatter_conv(const int32_t *table, int32_t K, int32_t identity_k, int64_t R, const void *X,
                     int32_t Cx, const float *W, int32_t Cw_in, int32_t Cw_out, int32_t transpose_w,
                     float *Y_accum, int32_t dtype, void *stream);

/* SparseMaxPool2d / 3d (csrc/pool.hip) ---------------------------------------------------------------
 * Replaces torch.ops.spconv.indice_maxpool / indice_maxpool_backward (spconv 1.2.1 functional.py SparseMaxPoolFunction;
 * the reference constructs no pool -- SURVEY.md A.5 -- but config strings can name one).  The rulebook is that of a
 * regular conv of the same geometry (or of a SubM one): the forward gathers through the by-output table, the backward
 * through the by-input table, as the convolutions do; no atomics, every row written once, fixed summation order.
 *     forward   Y[r, c]  = max(0, max_k X[table[k, r], c])      -- the output row starts at ZERO, as spconv's does:
 *                          for rows with negative entries this is NOT the plain maximum.  `x > y` decides, so NaN and
 *                          -0 never win; Y holds bit patterns of input elements or +0 in every dtype.
 *     backward  dX[j, c] = sum_k (X[j, c] == Y[o, c]) ? dY[o, c] : 0,  o = table[k, j] >= 0  -- ties all receive the
 *                          gradient, and so does a 0 under an output that stayed 0; fp32 sums in ascending k, rounded
 *                          once to the row type.
 * wfs_maxpool_fwd: table [K, R] by OUTPUT rows (nbr_in; for SubM nbr_out with its mirrored kmap_host -- a maximum does
 *   not depend on which offset a column stands for, the map only has to be a permutation); X [X_rows, C], Y [R, C].
 * wfs_maxpool_bwd: table by INPUT rows, dense [K, N] (packed_kl == 0) or the packed [K / packed_kl, N] of
 *   wfs_event_rulebook_conv when wfs_maxpool_packed_ok says so (same dX bit for bit); X / dX [N, C], Y / dY [M_rows, C].
 * Any C >= 1: rows of whole 16-byte pieces (C * sizeof(T) % 16 == 0) take vector kernels, every other C scalar ones.
 * r_dev / n_dev as everywhere: rows beyond the valid count are neither read nor written.  Table entries outside
 * [0, X_rows) / [0, M_rows) count as "no neighbour" (an overflowed build leaves such entries until its flag is read). */
int wfs_maxpool_fwd(const int32_t *table, const int32_t *kmap_host, int32_t K, int64_t R, const void *X, int64_t X_rows,
                    int32_t C, void *Y, int32_t dtype, const int64_t *r_dev, void *stream);
int wfs_maxpool_packed_ok(int32_t packed_kl, int32_t K, int32_t C, int32_t dtype);
int wfs_maxpool_bwd(const int32_t *table, int32_t K, int32_t packed_kl, int64_t N, const void *X, const void *Y,
                    const void *dY, int64_t M_rows, int32_t C, void *dX, int32_t dtype, const int64_t *n_dev, void *stream);

/* BatchNorm1d (+ReLU) over the active rows ------------------------------------------------------
 * What spconv.SparseSequential does with the plain nn.BatchNorm1d / nn.ReLU modules the reference
 * puts after every sparse conv (src/models/SPConvBlocks.py:505-508): applied to .features [N, C],
 * statistics over the N active rows.  Two launches per direction (column reduction into per-block partials;
 * elementwise pass whose blocks first fold the partials in a fixed order): deterministic, no atomics.
 * training != 0: batch statistics (biased variance), running_mean/var (may be NULL) updated with
 * `momentum` using the unbiased variance and *num_batches_tracked (device int64, may be NULL)
 * incremented, exactly as torch.  training == 0: running statistics.
 * relu != 0 fuses y = max(0, .).  save_mean / save_invstd [C] are outputs the backward consumes.
 * gamma / beta may be NULL (affine=False).  C <= 1024.                                           */
size_t wfs_bn_workspace_bytes(int64_t N, int32_t C);


int wfs_bn_relu_fwd(const void *X, int64_t N, int32_t C, const float *gamma, const float *beta,
                    float *running_mean, float *running_var, int64_t *num_batches_tracked,
                    float momentum, float eps,
                    int32_t training, int32_t relu, void *Y, float *save_mean, float *save_invstd,
                    void *workspace, size_t workspace_bytes, int32_t dtype, const int64_t *n_dev,
                    void *stream);

int wfs_bn_relu_bwd(const void *X, const void *dY, int64_t N, int32_t C, const float *gamma,
                    const float *beta, const float *save_mean, const float *save_invstd,
                    int32_t training, int32_t relu, void *dX, float *dgamma, float *dbeta,
                    void *workspace, size_t workspace_bytes, int32_t dtype, const int64_t *n_dev,
                    void *stream);

/* Which kernel family wfs_bn_relu_fwd (backward == 0) or wfs_bn_relu_bwd (backward != 0) runs for N rows of C channels
 * of `dtype`; host only, nothing is launched (the tests use it to know what a case covers).  Returns
 *   0  column-block kernels (wide layers with few rows)
 *   1  register-resident kernels; *rows_per_thread = rows a thread holds (2, 4, 8 or 16)
 *   2  loop kernels, four channels per thread        3  loop kernels, one channel per thread
 *   4  channel slices of at most 1024 channels
 *   -WFS_EINVAL (negative: 1 is taken) for a channel count, dtype or N < 0 that the entry points refuse.
 * *partials = the number of per-block partial sums the elementwise pass folds (0: none, the eval forward); both pointers
 * may be NULL, *rows_per_thread is 0 outside family 1.  Additions only: WFS_ABI_VERSION stays. */
int wfs_bn_plan(int64_t N, int32_t C, int32_t dtype, int32_t training, int32_t backward, int32_t *rows_per_thread,
                int32_t *partials);

/* After wfs_rulebook_emit of a regular conv whose site table was a direct grid: pointers into `workspace` to the
 * cell -> output row map of the build (ticket[cell] != 0xFFFFFFFF <=> the output cell b * out_volume + pos is active,
 * slot_id[cell] = its row).  Returns 1 and sets the pointers, or 0 when this build has no such map.  The map lives as
 * long as the workspace is kept. */
int wfs_rulebook_cell_map(const wfs_geometry *g, int64_t N, void *workspace, const uint32_t **ticket,
                          const int32_t **slot_id, int64_t *cells);

/* SparseConvTensor.dense() -------------------------------------------------------------------
 * Y is [B, C, *spatial] (channels first, contiguous) and must be zero-filled by the caller;
 * rows are assigned, not accumulated.  winner_ws: NULL when coordinates are unique, else int32
 * [B * volume] scratch that makes "the highest row wins" deterministic, as the reference's CPU
 * assignment order does (A.1).  wfs_to_dense_bwd gathers dX[m,c] = dY[b,c,pos] for every row. */
int wfs_to_dense(const void *X, const int32_t *indices, int64_t M, int32_t ndim,
                 const int32_t *spatial_host, int32_t batch_size, int32_t C, void *Y,
                 int32_t *winner_ws, int32_t dtype, const int64_t *m_dev, void *stream);

int wfs_to_dense_bwd(const void *dY, const int32_t *indices, int64_t M, int32_t ndim,
                     const int32_t *spatial_host, int32_t batch_size, int32_t C, void *dX,
                     int32_t dtype, const int64_t *m_dev, void *stream);

/* dense() and its backward through a cell -> row map (wfs_rulebook_cell_map of the conv that produced the rows, whose
 * coordinates are unique by construction).  Y [B, C, V] need NOT be zero-filled: every cell is written, a block owns 64
 * cells of one event and stores whole runs per channel.  V = out volume; C % 4 == 0, C <= 128, V even for 16-bit rows;
 * rows with id >= the valid count (m_dev) are treated as absent. */
int wfs_to_dense_mapped(const void *X, const uint32_t *ticket, const int32_t *slot_id, int64_t M,
                        const int64_t *m_dev, int32_t batch_size, int64_t V, int32_t C, void *Y, int32_t dtype,
                        void *stream);

int wfs_to_dense_bwd_mapped(const void *dY, const uint32_t *ticket, const int32_t *slot_id, int64_t M,
                            const int64_t *m_dev, int32_t batch_size, int64_t V, int32_t C, void *dX, int32_t dtype,
                            void *stream);

/* The head straight off the sparse rows (round 4; csrc/shead.hip).
 * Replaces the whole tail spconv.ToDense -> view(-1, n_linear) -> nn.Linear(n_linear, n_type) of the reference's
 * SPConvNet (src/models/SPConvNet.py:65-68; one-layer LinearBlock, src/models/ConvBlocks.py:82-102) AND its backward,
 * without materialising the dense tensor:
 *     Y[b][o]  = bias[o] + sum over rows i of event b, channels c:  X[i][c] * W[o][c * V + cell(i)]
 *     dX[i][c] = sum_o G[b(i)][o] * W[o][c * V + cell(i)];   dW[o][c * V + cell] = sum_b G[b][o] * X[row(b, cell)][c]
 * X [M, C] rows of the last conv's output (dtype), (ticket, slot_id) = that conv's cell -> row map (wfs_rulebook_cell_map,
 * or wfs_event_rulebook_conv's cell_row passed as both), V = its out volume, W fp32 [O, C * V] = nn.Linear.weight as it
 * is (channels first over the grid), Y / G fp32 [batch, O].  Cell-major kernels: a lane owns a cell, reads its weights
 * coalesced in the parameter's own layout and walks the events through the map.  O <= 4, C % 8 == 0, C <= 64
 * (wfs_sparse_head_ok).  dX / dW may be NULL; dB comes with dW.  defer as in wfs_gather_dw (the per-slice dW partials
 * then join the step's deferred slab reduction).  Deterministic (no atomics, fixed orders). */
int wfs_sparse_head_ok(int32_t batch, int64_t V, int32_t C, int32_t O, int32_t dtype);
size_t wfs_sparse_head_workspace_bytes(int32_t batch, int64_t V, int32_t C, int32_t O);
int wfs_sparse_head_fwd(const void *X, const uint32_t *ticket, const int32_t *slot_id, int64_t M,
                        const int64_t *m_dev, int32_t batch, int64_t V, int32_t C, const float *W,
                        const float *bias, int32_t O, float *Y, int32_t dtype, void *workspace,
                        size_t workspace_bytes, void *stream);
int wfs_sparse_head_bwd(const void *X, const float *G, const uint32_t *ticket, const int32_t *slot_id,
                        int64_t M, const int64_t *m_dev, int32_t batch, int64_t V, int32_t C, const float *W,
                        int32_t O, void *dX, float *dW, float *dB, int32_t dtype, void *workspace,
                        size_t workspace_bytes, wfs_dw_job *defer, void *stream);

/* classification head -----------------------------------------------------------------------
 * The reference flattens ToDense's output and applies the LinearBlock (src/models/SPConvNet.py:67-68,
 * src/models/ConvBlocks.py:82-102); the final nn.Linear has n_type = 2..4 outputs over tens of
 * thousands of inputs, a streaming problem rather than a GEMM.  X [B, I] fp32 or bf16 (dtype),
 * W [O, I] fp32 (nn.Linear.weight), Y / G [B, O] fp32, 1 <= O <= 8.  Rows with I % 8 == 0 and I >= 1024 stream
 * through vector kernels; any other row length (the short second layer of a two-layer head) takes scalar ones.
 *     Y = X W^T + bias;   dX = G W (X's dtype);   dW = G^T X (deterministic chunked reduction).
 * dX or dW may be NULL to skip that product; dB [O] (optional, computed with dW) = sum_b G[b][:].      */
size_t wfs_head_workspace_bytes(int64_t B, int64_t I, int32_t O);

int wfs_head_fwd(const void *X, int64_t B, int64_t I, const float *W, const float *bias, int32_t O,
                 float *Y, int32_t dtype, void *stream);

/* defer (optional): as in wfs_gather_dw -- when dX and dW are both asked for, the sum over the dW partials may be left
 * to a later wfs_dw_reduce_jobs (defer->nslabs > 0 on return; dW not written yet, the workspace must stay alive). */
int wfs_head_bwd(const void *X, const float *G, int64_t B, int64_t I, const float *W, int32_t O,
                 void *dX, float *dW, float *dB, int32_t dtype, void *workspace, size_t workspace_bytes,
                 wfs_dw_job *defer, void *stream);


/* dropout generator (the three waveform front ends below; csrc/wfs_rows.h) ------------------------------------
 * dropout_p in [0, 1) and seed_dev = one int64 in DEVICE memory (drawn by the caller, e.g. torch.randint, so that a
 * captured graph gets a fresh seed per replay).  Every element that a front end drops out has a 64-bit counter ctr,
 * unique per element (the layout is given with each front end), and
 *     z = splitmix64-finaliser(seed + ctr * 0x9E3779B97F4A7C15)
 * (xor-shift 30, * 0xBF58476D1CE4E5B9, xor-shift 27, * 0x94D049BB133111EB, xor-shift 31); the element is dropped when
 * z >> 32 < (uint32)(p * 2^32), else scaled by the fp32 1 / (1 - p).  No mask is stored: every later pass, the backward's
 * included, rebuilds it from the seed (pass the forward's p and seed to the backward).  dropout_p == 0 (seed_dev may be
 * NULL) is the eval-mode identity.  Same distribution as nn.Dropout, not the same bits. */

/* hybrid front end -----------------------------------------------------------------------------------
 * TemporalConvNet(1, [1] * levels, kernel_size = k) as the reference's SPConvNet applies it to the waveform rows
 * before the sparse stack (src/models/SPConvNet.py:56-61,83-92; src/models/ConvBlocks.py:114-173): per level i two
 * causal k-tap FIR filters with dilation 2^i, ReLU after each, residual + ReLU.  One launch per direction; a row
 * [L] stays in LDS through all levels.  X, Y, dY, dX [N, L] fp32 or bf16 (dtype); taps [levels][2][k] and bias
 * [levels][2] are the EFFECTIVE filter taps (after weight norm) in DEVICE memory, fp32.  levels <= 8, k <= 8,
 * L <= 4096; the backward needs wfs_tcn_lds_bytes(L, levels, 1) <= 150 KiB (else WFS_EINVAL: use another path).
 * wfs_tcn_bwd writes per-row partial sums partial[N][levels][2][k + 1] (taps, then the bias); their sum over rows is
 * d loss / d (taps, bias).
 * Dropout (the nn.Dropout(p) after each of a level's two ReLUs, ConvBlocks.py:125-134): the dropout generator above;
 * element (row n, conv c = 2 * level + {0, 1} (c < 2^4), sample t (t < 2^12)) has the counter
 *     ctr = n << 16 | c << 12 | t                                                                        */
size_t wfs_tcn_lds_bytes(int32_t L, int32_t levels, int32_t backward);

int wfs_tcn_fwd(const void *X, int64_t N, int32_t L, const float *taps, const float *bias, int32_t levels,
                int32_t k, void *Y, int32_t dtype, float dropout_p, const int64_t *seed_dev, void *stream);

int wfs_tcn_bwd(const void *X, const void *dY, int64_t N, int32_t L, const float *taps, const float *bias,
                int32_t levels, int32_t k, void *dX, float *partial, int32_t dtype, float dropout_p,
                const int64_t *seed_dev, void *stream);

/* Weight norm of the front end's taps (torch.nn.utils.weight_norm around every Conv1d of the reference's TemporalBlock,
 * src/models/ConvBlocks.py:118-131: w = g v / |v|), all convolutions in one launch each way.  param_ptrs: device array
 * of n_conv records of six device addresses {v [k], g [1], b [1] or 0, dv [k], dg [1], db [1] (each 0 = not wanted)},
 * convolution c = 2 * level + which.  wfs_tcn_taps_fwd fills taps [n_conv][k] and bias [n_conv] as wfs_tcn_fwd / _bwd
 * take them; wfs_tcn_taps_bwd sums wfs_tcn_bwd's partial [N][n_conv][k + 1] over the rows (fixed order) and writes
 * dv, dg, db.  n_conv <= 16, k <= 8.                                                                                  */
int wfs_tcn_taps_fwd(const void *param_ptrs, int32_t n_conv, int32_t k, float *taps, float *bias, void *stream);
int wfs_tcn_taps_bwd(const void *param_ptrs, int32_t n_conv, int32_t k, const float *partial, int64_t N, void *stream);

/* multi-channel front end (csrc/tcnc.hip) ----------------------------------------------------------------
 * TemporalConvNet(c0, channels[0 .. levels-1], kernel_size = k) as the reference's TemporalWaveformNet builds it
 * (src/models/WaveformModels.py:8-45, TemporalBlock of src/models/ConvBlocks.py:114-152): level i (dilation 2^i) is
 * drop(relu(conv1)), drop(relu(conv2)), + residual (the 1x1 downsample when its input and output channels differ), relu.
 * X / Y [N][c0 | channels[levels-1]][L] in `dtype`; fp32 arithmetic.  channels is a HOST array.  Bounds: 1 <= every
 * channel count <= WFS_TCNC_MAX_CHANNELS, 2 <= k <= WFS_TCNC_MAX_K (k = 1 has no causal padding to chomp), 1 <= levels <= WFS_TCNC_MAX_LEVELS,
 * 1 <= L <= WFS_TCNC_MAX_L; wfs_tcnc_ok says WFS_OK or WFS_EINVAL (and every entry point refuses the same shapes).
 * param_ptrs: DEVICE array of wfs_tcnc_n_conv() records of six device addresses {v, g, b, dv, dg, db}, convolutions in
 * parameter order: per level conv1 (weight_v [cout][cin][k], weight_g [cout], bias [cout]), conv2 (the same with cin =
 * cout), then the downsample when cin != cout (its weight [cout][cin] as v, g = 0: no weight norm).  A gradient address
 * 0 is not written.
 * wfs_tcnc_taps_fwd: effective weights w = g v / |v| (norm over (cin, k) per output channel) into wts
 *   [wfs_tcnc_weights_floats] fp32 -- one launch, no host round trip.
 * wfs_tcnc_fwd: Y, and `saved` [wfs_tcnc_saved_floats] fp32 for the backward: per level relu(conv1) and relu(conv2)
 *   BEFORE dropout, and the level output.
 * wfs_tcnc_bwd: dX (dtype) from dY (dtype) and `saved`, and d weight_v / weight_g / bias / downsample straight into the
 *   gradient slots of param_ptrs; workspace [wfs_tcnc_bwd_workspace_floats] fp32.  Deterministic (fixed-order partial
 *   sums, no atomics).  N >= 1.
 * Dropout: the dropout generator above, after each of a level's two ReLUs; element (row n, conv c = 2 * level + {0, 1},
 * channel ch of that conv's output (ch < 2^5), sample t) has the counter
 *     ctr = (((n << 4 | c) << 5 | ch) << 12) | t
 * wfs_tcnc_fwd's second conv of a level and every mask pass of wfs_tcnc_bwd rebuild the masks from the seed.  */
#define WFS_TCNC_MAX_CHANNELS 32
#define WFS_TCNC_MAX_K 8
#define WFS_TCNC_MAX_LEVELS 8
#define WFS_TCNC_MAX_L 4096
int wfs_tcnc_ok(int32_t c0, const int32_t *channels, int32_t levels, int32_t k, int32_t L, int32_t dtype);
int wfs_tcnc_n_conv(int32_t c0, const int32_t *channels, int32_t levels, int32_t k);
size_t wfs_tcnc_weights_floats(int32_t c0, const int32_t *channels, int32_t levels, int32_t k);
size_t wfs_tcnc_saved_floats(int64_t N, int32_t L, int32_t c0, const int32_t *channels, int32_t levels);
size_t wfs_tcnc_bwd_workspace_floats(int64_t N, int32_t L, int32_t c0, const int32_t *channels, int32_t levels,
                                     int32_t k);
int wfs_tcnc_taps_fwd(const void *param_ptrs, int32_t c0, const int32_t *channels, int32_t levels, int32_t k,
                      float *wts, void *stream);
int wfs_tcnc_fwd(const void *X, int64_t N, int32_t L, int32_t c0, const int32_t *channels, int32_t levels, int32_t k,
                 const float *wts, float *saved, void *Y, int32_t dtype, float dropout_p, const int64_t *seed_dev,
                 void *stream);
int wfs_tcnc_bwd(const void *X, const void *dY, int64_t N, int32_t L, int32_t c0, const int32_t *channels,
                 int32_t levels, int32_t k, const float *wts, const float *saved, void *dX, float *workspace,
                 const void *param_ptrs, int32_t dtype, float dropout_p, const int64_t *seed_dev, void *stream);

/* dense Conv1d + BatchNorm1d + ReLU stack (csrc/conv1d.hip) -------------------------------------------------
 * The reference's Conv1DNet (src/models/ConvBlocks.py:176-217), the front end of ConvWaveformNet: per layer i of
 * `layers`, nn.Conv1d(c[i], channels[i], fs[i], stride = st[i], padding = pd[i]) with bias (non-causal, zero padded,
 * dilation 1), nn.BatchNorm1d(channels[i]) with affine parameters and running statistics, nn.ReLU; c[0] = c0,
 * c[i + 1] = channels[i]; L[i + 1] = (L[i] + 2 pd[i] - fs[i]) / st[i] + 1.  ONE call covers the whole stack:
 * X [N][c0][L] -> Y [N][channels[layers-1]][L[layers]] in `dtype`; fp32 arithmetic, statistics in fp64.
 * channels / fs / st / pd / momentum / eps are HOST arrays of `layers` entries.  Bounds: every channel count in
 * 1 .. WFS_CONV1D_MAX_CHANNELS, 1 <= fs <= WFS_CONV1D_MAX_K, 1 <= st <= WFS_CONV1D_MAX_STRIDE, 0 <= pd < fs,
 * 1 <= layers <= WFS_CONV1D_MAX_LAYERS, 1 <= L <= WFS_CONV1D_MAX_L, every L[i] >= 1; wfs_conv1d_ok says WFS_OK or
 * WFS_EINVAL (and every entry point refuses the same shapes).
 * param_ptrs: DEVICE array of `layers` records of fourteen device addresses: {conv.weight [cout][cin][fs], conv.bias
 * [cout] or 0, bn.weight, bn.bias, running_mean, running_var (fp32 [cout]), num_batches_tracked (int64 [1] or 0)},
 * then the gradient addresses of the first four and three unused words.  A gradient address 0 is not written.
 * n_valid_dev: DEVICE count of valid rows (NULL: all N).  Rows at or beyond it are never read: they add nothing to
 * the batch statistics or to any parameter gradient, and get Y = 0 and dX = 0.
 * wfs_conv1d_fwd: layers + 1 launches.  training != 0: batch statistics per channel over n_valid x L[i + 1] elements
 *   (biased variance), and running_mean / running_var (unbiased, momentum[i]) / num_batches_tracked updated on the
 *   device; training == 0: the running statistics.  `saved` [wfs_conv1d_saved_floats] fp32 keeps every layer's pre-BN
 *   convolution output and the statistics used, for the backward.  An empty batch (n_valid <= 0) in a training call
 *   folds mean 0 and variance 0 into the running statistics and counts a batch; torch raises there.
 * wfs_conv1d_bwd: layers + 2 launches.  dX (dtype; NULL: not wanted) from dY (dtype) and `saved`; d conv.weight,
 *   d conv.bias, d bn.weight, d bn.bias straight into the gradient slots; workspace [wfs_conv1d_bwd_workspace_floats]
 *   fp32.  `training` as in the forward call.  Deterministic (fixed-order partial sums, no atomics).  N >= 1.  */
#define WFS_CONV1D_MAX_CHANNELS 64
#define WFS_CONV1D_MAX_K 16
#define WFS_CONV1D_MAX_STRIDE 8
#define WFS_CONV1D_MAX_LAYERS 8
#define WFS_CONV1D_MAX_L 4096
int wfs_conv1d_ok(int32_t c0, const int32_t *channels, const int32_t *fs, const int32_t *st, const int32_t *pd,
                  int32_t layers, int32_t L, int32_t dtype);
size_t wfs_conv1d_saved_floats(int64_t N, int32_t L, int32_t c0, const int32_t *channels, const int32_t *fs,
                               const int32_t *st, const int32_t *pd, int32_t layers);
size_t wfs_conv1d_bwd_workspace_floats(int64_t N, int32_t L, int32_t c0, const int32_t *channels, const int32_t *fs,
                                       const int32_t *st, const int32_t *pd, int32_t layers);
int wfs_conv1d_fwd(const void *X, int64_t N, int32_t L, int32_t c0, const int32_t *channels, const int32_t *fs,
                   const int32_t *st, const int32_t *pd, int32_t layers, const void *param_ptrs, const float *momentum,
                   const float *eps, int32_t training, float *saved, void *Y, int32_t dtype, const int64_t *n_valid_dev,
                   void *stream);
int wfs_conv1d_bwd(const void *X, const void *dY, int64_t N, int32_t L, int32_t c0, const int32_t *channels,
                   const int32_t *fs, const int32_t *st, const int32_t *pd, int32_t layers, const void *param_ptrs,
                   int32_t training, const float *saved, void *dX, float *workspace, int32_t dtype,
                   const int64_t *n_valid_dev, void *stream);
/* Host only, launches nothing: the plan the two calls above follow, for the tests.  out[layers][10] = {L_in, L_out,
 * position blocks of the forward (and head) pass over N L_out, position blocks of the input-gradient role over N L_in
 * (as launched when that gradient is wanted), its input-channel chunks, dW blocks per column chunk, column chunks of
 * the cin fs + 1 dW columns, columns of the last chunk, thread groups of the last chunk, accumulator width CO}, then
 * out[layers * 10] = blocks of the last forward launch.  WFS_EINVAL where wfs_conv1d_ok refuses the plan (and for a row
 * count the size queries answer 0 to, and out == NULL).  Additions only: WFS_ABI_VERSION stays. */
int wfs_conv1d_arms(int64_t N, int32_t L, int32_t c0, const int32_t *channels, const int32_t *fs, const int32_t *st,
                    const int32_t *pd, int32_t layers, int32_t *out);

/* dense Conv2d + BatchNorm2d + ReLU (+ Dropout) stack on event maps (csrc/conv2d.hip) ------------------------
 * The reference's Conv2DBlock (src/models/ConvBlocks.py:220-289) under DenseConvNet: per layer i of `layers`,
 * nn.Conv2d(c[i], channels[i], (fs, fs), (st, st), pd, (dil, dil)) with or without bias (zero padded),
 * nn.BatchNorm2d(channels[i]) with affine parameters and running statistics, nn.ReLU, and nn.Dropout(dropout_p[i])
 * where dropout_p[i] > 0; c[0] = c0, H[i + 1] = (H[i] + 2 pd - dil (fs - 1) - 1) / st + 1, W alike.  ONE call covers the
 * whole stack.  X is channels-LAST, [B][H][W][c0] (what wfs_densify_rows writes; torch's channels_last memory format of
 * an NCHW tensor); Y and dY are channels-FIRST, [B][channels[layers-1]][H'][W'] (the order the reference flattens); dX
 * is channels-last like X.  All in `dtype`.  fp32 accumulation on the matrix cores (16-bit rows: 16-bit MFMA; the
 * forward keeps the filters in three and the activations between layers in two 16-bit pieces so that the ReLU masks
 * are those of an fp32 run, the backward rounds the filters and the gradients between layers to the row type; fp32
 * rows: v_mfma_f32_32x32x2_f32, an fp32 FMA chain); statistics in fp64.
 * channels / fs / st / pd / dil / momentum / eps / dropout_p are HOST arrays of `layers` entries (dropout_p NULL: none).
 * Bounds: channel counts 1 .. WFS_CONV2D_MAX_CHANNELS, 1 <= fs <= WFS_CONV2D_MAX_K, 1 <= st <= WFS_CONV2D_MAX_STRIDE,
 * 1 <= dil <= WFS_CONV2D_MAX_DILATION, 0 <= pd <= dil (fs - 1), 1 <= layers <= WFS_CONV2D_MAX_LAYERS,
 * 1 <= H, W <= WFS_CONV2D_MAX_HW, every layer's output >= 1 x 1, 1 <= B <= WFS_CONV2D_MAX_BATCH, and for a training
 * call B H' W' >= 2 at every layer (torch raises below that); wfs_conv2d_ok says WFS_OK or WFS_EINVAL (and every entry
 * point refuses the same shapes).
 * param_ptrs: DEVICE array of `layers` records of fourteen device addresses: {conv.weight [cout][cin][fs][fs],
 * conv.bias [cout] or 0, bn.weight, bn.bias, running_mean, running_var (fp32 [cout]), num_batches_tracked (int64 [1]
 * or 0)}, then the gradient addresses of the first four and three unused words.  A gradient address 0 is not written.
 * wfs_conv2d_fwd: 3 layers + 1 launches (training) or 2 layers + 1 (eval).  training != 0: batch statistics per channel
 *   over B H' W' elements (biased variance), running_mean / running_var (unbiased, momentum[i]) / num_batches_tracked
 *   updated on the device, dropout applied; training == 0: the running statistics, no dropout.  `saved`
 *   [wfs_conv2d_saved_floats] fp32 keeps every layer's pre-BN convolution output (fp32), the statistics used, the
 *   activations between the layers (row type) and the repacked filters, for the backward.
 * wfs_conv2d_bwd: 4 layers + 1 launches, one more when dX is wanted (dX NULL: the first layer's input gradient is not
 *   computed).  d conv.weight, d conv.bias, d bn.weight, d bn.bias straight into the gradient slots; workspace
 *   [wfs_conv2d_bwd_workspace_floats] fp32.  `training`, dropout_p and seed_dev as in the forward call.  Deterministic
 *   (fixed-order partial sums, no float atomics).
 * Dropout: the dropout generator above; element (event b, channel c, y, x) of layer l's output has the counter
 *       ctr = l << 44 | ((b C_l + c) H_l + y) W_l + x        (the element's flat index in the layer's output as NCHW)
 *   Nothing is stored: the backward rebuilds the masks from the seed.
 * wfs_densify_rows: rows [n_cap][C] (dtype) at coords int32 [n_cap][3] = (x, y, event) -> out [B][H][W][C], every cell
 *   written by ONE launch (cells without a row: zeros; no memset needed).  Rows at or beyond *n_valid_dev (NULL: all
 *   n_cap) are never read; a row whose coordinate lies outside [0, H) x [0, W) x [0, B) is skipped and never
 *   dereferenced.  Rows with EQUAL coordinates are summed (as to_dense does), in row order, in fp32, rounded once: no
 *   float atomics, the result does not depend on scheduling.  No backward: the rows are inputs.
 * Nothing here allocates, synchronises or reads back: every launch goes to `stream` (capturable).  */
#define WFS_CONV2D_MAX_CHANNELS 512
#define WFS_CONV2D_MAX_K 5
#define WFS_CONV2D_MAX_STRIDE 3
#define WFS_CONV2D_MAX_DILATION 4
#define WFS_CONV2D_MAX_LAYERS 8
#define WFS_CONV2D_MAX_HW 32
#define WFS_CONV2D_MAX_BATCH 2048
int wfs_conv2d_ok(int32_t c0, const int32_t *channels, const int32_t *fs, const int32_t *st, const int32_t *pd,
                  const int32_t *dil, int32_t layers, int64_t B, int32_t H, int32_t W, int32_t training, int32_t dtype);
size_t wfs_conv2d_saved_floats(int64_t B, int32_t H, int32_t W, int32_t c0, const int32_t *channels, const int32_t *fs,
                               const int32_t *st, const int32_t *pd, const int32_t *dil, int32_t layers, int32_t dtype);
size_t wfs_conv2d_bwd_workspace_floats(int64_t B, int32_t H, int32_t W, int32_t c0, const int32_t *channels,
                                       const int32_t *fs, const int32_t *st, const int32_t *pd, const int32_t *dil,
                                       int32_t layers, int32_t dtype);
/* What wfs_conv2d_fwd / wfs_conv2d_bwd do with every layer of a plan; host only, nothing is launched (the tests use
 * it to know what a case covers).  out[layers][8] = {M = B H' W', row blocks of the statistics / g-sum / dz passes,
 * row blocks of the BN + ReLU pass, forward GEMM tiles along M, along N, its K steps, dW slices, positions in the last
 * slice}.  WFS_EINVAL where wfs_conv2d_ok refuses the shape for an eval call, and for out == NULL.  Additions only:
 * WFS_ABI_VERSION stays. */
int wfs_conv2d_arms(int64_t B, int32_t H, int32_t W, int32_t c0, const int32_t *channels, const int32_t *fs,
                    const int32_t *st, const int32_t *pd, const int32_t *dil, int32_t layers, int32_t dtype,
                    int32_t *out);
int wfs_conv2d_fwd(const void *X, int64_t B, int32_t H, int32_t W, int32_t c0, const int32_t *channels, const int32_t *fs,
                   const int32_t *st, const int32_t *pd, const int32_t *dil, int32_t layers, const void *param_ptrs,
                   const float *momentum, const float *eps, const float *dropout_p, const int64_t *seed_dev,
                   int32_t training, float *saved, void *Y, int32_t dtype, void *stream);
int wfs_conv2d_bwd(const void *X, const void *dY, int64_t B, int32_t H, int32_t W, int32_t c0, const int32_t *channels,
                   const int32_t *fs, const int32_t *st, const int32_t *pd, const int32_t *dil, int32_t layers,
                   const void *param_ptrs, const float *dropout_p, const int64_t *seed_dev, int32_t training,
                   const float *saved, void *dX, float *workspace, int32_t dtype, void *stream);
int wfs_densify_rows(const void *rows, const int32_t *coords, int64_t n_cap, int32_t C, int64_t B, int32_t H, int32_t W,
                     const int64_t *n_valid_dev, void *out, int32_t dtype, void *stream);

/* recurrent front end (csrc/rnn.hip) ------------------------------------------------------------------------
 * torch.nn.RNN(I, H, layers, nonlinearity, bias, dropout, bidirectional, batch_first=True) as the reference's
 * RecurrentNet builds it (src/models/RecurrentBlocks.py): per layer l and direction d (0 forward in t, 1 backward)
 *   h[t] = act(W_ih in_l[t] + b_ih + W_hh h[t -+ 1] + b_hh), h[start] = 0;  in_0 = X, in_l = drop(out_{l-1}),
 *   out_l[t] = h[t] of direction 0 then of direction 1;  Y = out_{layers-1}.
 * X [N][T][I], Y / dY [N][T][dirs H], dX [N][T][I], hidden [layers dirs][N][H] in `dtype`; parameters, arithmetic and
 * saved state fp32.  Bounds: 1 <= I <= WFS_RNN_MAX_INPUT, 1 <= H <= WFS_RNN_MAX_HIDDEN, 1 <= layers <=
 * WFS_RNN_MAX_LAYERS, dirs 1 or 2, 1 <= T <= WFS_RNN_MAX_T, nonlinearity WFS_RNN_RELU or WFS_RNN_TANH; wfs_rnn_ok says
 * WFS_OK or WFS_EINVAL (and every entry point refuses the same shapes).
 * param_ptrs: DEVICE array of wfs_rnn_n_params() = layers dirs records of eight device addresses
 *   {w_ih, w_hh, b_ih, b_hh, dw_ih, dw_hh, db_ih, db_hh}, record layer * dirs + d, torch's shapes: w_ih [H][I] (layer 0)
 *   or [H][dirs H], w_hh [H][H], biases [H] (0: no bias).  A gradient address 0 is not written.
 * wfs_rnn_fwd: Y, hidden (may be NULL: not written) and `saved` [wfs_rnn_saved_floats] fp32 for the backward -- opaque:
 *   X and every layer's outputs before dropout, lane-contiguous ([t][channel][N rounded up to 64]).
 * wfs_rnn_bwd: dX (may be NULL: not computed) from dY and `saved`, and every parameter gradient straight into the
 *   gradient slots of param_ptrs; workspace [wfs_rnn_bwd_workspace_floats] fp32.  Deterministic (fixed-order partial
 *   sums, no atomics).  N >= 1.  (The gradient of `hidden` is not an input: hidden is an output for inspection only.)
 * Dropout: torch's placement -- the outputs of every layer but the last -- with the dropout generator above (p = 0 in
 *   eval mode); element (row n, layer l, channel c of out_l (c < dirs H <= 64), sample t) has the counter
 *       ctr = (((n << 3 | l) << 6 | c) << 12) | t
 *   The next layer's passes and the backward rebuild the mask from the seed.
 * Nothing here allocates, synchronises or reads back: every launch goes to `stream` (capturable).  */
#define WFS_RNN_MAX_INPUT 32
#define WFS_RNN_MAX_HIDDEN 32
#define WFS_RNN_MAX_LAYERS 8
#define WFS_RNN_MAX_T 4096
#define WFS_RNN_RELU 0
#define WFS_RNN_TANH 1
int wfs_rnn_ok(int32_t I, int32_t H, int32_t layers, int32_t dirs, int32_t nonlinearity, int32_t T, int32_t dtype);
int wfs_rnn_n_params(int32_t layers, int32_t dirs);
size_t wfs_rnn_saved_floats(int64_t N, int32_t T, int32_t I, int32_t H, int32_t layers, int32_t dirs);
size_t wfs_rnn_bwd_workspace_floats(int64_t N, int32_t T, int32_t I, int32_t H, int32_t layers, int32_t dirs);
int wfs_rnn_fwd(const void *X, int64_t N, int32_t T, int32_t I, int32_t H, int32_t layers, int32_t dirs,
                int32_t nonlinearity, const void *param_ptrs, float *saved, void *Y, void *hidden, int32_t dtype,
                float dropout_p, const int64_t *seed_dev, void *stream);
int wfs_rnn_bwd(const void *dY, int64_t N, int32_t T, int32_t I, int32_t H, int32_t layers, int32_t dirs,
                int32_t nonlinearity, const void *param_ptrs, const float *saved, void *dX, float *workspace,
                int32_t dtype, float dropout_p, const int64_t *seed_dev, void *stream);

/* waveform rows -> voxels (csrc/voxelize.hip) ---------------------------------------------------------
 * The hand-over between the front end and a 3-D sparse stack (BASELINE configs[4]: feat [n, 1, 2T] -> TCN -> voxelise ->
 * SubM3d head; the reference's 3-D datasets are voxelised offline, src/datasets/PulseDataset.py:543-625).  Row r of
 * `rows` [n_cap, 2T] (left PMT samples, then right) has an ACTIVE sample t iff rows[r][t] > threshold ||
 * rows[r][T + t] > threshold; every active (r, t) is one voxel, numbered row-major, t ascending (the order of the host
 * 3-D layout: psd/synthetic.py; deterministic, no atomics: a ballot per 64 samples and a prefix over the rows).
 *   coords     int32 [n_cap, 3] = (x, y, evt) -- the 2-D layout's column order
 *   n_dev      valid rows as everywhere (NULL = n_cap); rows beyond it give no voxel whatever they hold
 *   rows / values / feats / dfeat / dY share `dtype`; `values` (e.g. the TCN's output, may be `rows` itself) gives the
 *   features; 1 <= T <= WFS_VOXELIZE_MAX_SAMPLES, n_cap * T < 2^31.
 * wfs_voxelize_plan (two launches): row_offsets int32 [wfs_voxelize_offsets_ints(n_cap, T)] = exclusive voxel offset of
 *   every 64-sample slice of every row (S = ceil(T / 64) per row; row r's voxels start at row_offsets[r * S], rows beyond
 *   the valid count have none), row_offsets[n_cap * S] = V, the true voxel count; *v_dev (int64, device) = min(V, V_cap);
 *   *overflow_dev = 1 if V > V_cap -- STICKY, set and never cleared, as wfs_rulebook_emit's.  event_offsets (may be
 *   NULL; needs coords and batch_size): the wfs_event_offsets table of the voxels, taken from the offsets of each event's
 *   first row (flag word 0 != 0 <=> the rows' evt column is not non-decreasing / in [0, batch_size)).  An eager caller
 *   passes V_cap = n_cap * T, reads *v_dev back once and emits into exactly that many rows.
 * wfs_voxelize_emit (one launch): indices int32 [V_cap, 4] = (evt, x, y, t), batch-first; feats [V_cap, 2] =
 *   (values[r][t], values[r][T + t]); voxels beyond V_cap are not written.  Same rows, coords and threshold as the plan.
 * wfs_voxelize_bwd (one launch): dY [n_cap, 2T] from dfeat [V_cap, 2] through the plan's row_offsets and the t column of
 *   the emitted indices: dY[r][t] / dY[r][T + t] = dfeat of the voxel (r, t), EXACT ZEROS everywhere else -- every row
 *   up to the capacity is written whole (wfs_tcn_bwd has no row count and sums its tap partials over padding rows too). */
#define WFS_VOXELIZE_MAX_SAMPLES 4096
size_t wfs_voxelize_offsets_ints(int64_t n_cap, int32_t T);
int wfs_voxelize_plan(const void *rows, const int32_t *coords, int64_t n_cap, int32_t T, const int64_t *n_dev,
                      float threshold, int32_t batch_size, int64_t V_cap, int32_t *row_offsets, int64_t *v_dev,
                      int32_t *event_offsets, int32_t *overflow_dev, int32_t dtype, void *stream);
int wfs_voxelize_emit(const void *rows, const void *values, const int32_t *coords, int64_t n_cap, int32_t T,
                      float threshold, const int32_t *row_offsets, int64_t V_cap, int32_t *indices, void *feats,
                      int32_t dtype, void *stream);
int wfs_voxelize_bwd(const void *dfeat, const int32_t *indices, const int32_t *row_offsets, int64_t n_cap, int32_t T,
                     int64_t V_cap, void *dY, int32_t dtype, void *stream);

/* loss ---------------------------------------------------------------------------------------------
 * torch.nn.CrossEntropyLoss(reduction='mean') as the reference's LitPSD applies it to the [B, n_type] logits
 * (src/engineering/LitBase.py:38-43, LitPSD.py:102), forward AND d loss / d logits in one launch (torch runs six:
 * log_softmax, nll_loss, their backwards and two fills).  logits fp32 [B, C], target int64 [B]; rows whose target
 * equals ignore_index are skipped and do not count in the mean (torch's default is -100).
 * loss: device float [1]; dlogits [B, C] = (softmax - onehot) / counted rows, or NULL for the forward alone. */
int wfs_xent_mean_fwd_bwd(const float *logits, const int64_t *target, int64_t B, int32_t C,
                          int64_t ignore_index, float *loss, float *dlogits, void *stream);

/* optimizer ----------------------------------------------------------------------------------------
 * torch.optim.SGD's update (the optimizer of the reference's example configs, config/examples/GEP.json:51-69, built
 * by src/engineering/LitPSD.py:60-76) on one flat fp32 parameter buffer in a single launch; arithmetic and order of
 * torch/optim/sgd.py.  lr is read from device memory so that a scheduler can change it under a captured graph.
 * momentum_buf may be NULL when momentum == 0; first_step != 0 initialises it with the gradient, as torch does. */
int wfs_sgd_step(float *param, const float *grad, float *momentum_buf, int64_t n, const float *lr_dev,
                 float momentum, float dampening, float weight_decay, int32_t nesterov, int32_t first_step,
                 void *stream);

/* torch.optim.Adam / AdamW's update (optimizer_class "optim.Adam" / "optim.AdamW", built by
 * src/engineering/LitPSD.py:60-76) on one flat fp32 parameter buffer of n elements; arithmetic and order of
 * torch/optim/adam.py _single_tensor_adam with capturable=False (maximize, L2 or decoupled weight decay, lerp of
 * exp_avg, mul + addcmul of exp_avg_sq, bias corrections in double, amsgrad's running maximum, addcdiv).  Two launches:
 * a one-thread prologue advances the step and computes the step's coefficients, then the elementwise update.
 * hyper_dev: device doubles {lr, beta1, beta2, eps, weight_decay}, read by every call so that a scheduler reaches a
 * captured graph.  step_dev: torch's state["step"] as a device float; the call computes with step + 1 and stores it.
 * coef_dev: device workspace of WFS_ADAM_COEF_FLOATS floats (4-byte aligned) that the call writes and reads.
 * max_exp_avg_sq may be NULL when amsgrad == 0.  decoupled != 0 is AdamW.  n == 0 still advances the step. */
#define WFS_ADAM_COEF_FLOATS 16
int wfs_adam_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, float *max_exp_avg_sq,
                  int64_t n, const double *hyper_dev, float *step_dev, float *coef_dev, int32_t amsgrad,
                  int32_t maximize, int32_t decoupled, void *stream);

/* batch hand-over -------------------------------------------------------------------------------------
 * One launch that places a device-resident batch into the fixed buffers a captured step reads: coords [n, cols]
 * int32 (copied as is to coords_dst and, columns permuted by perm_host, to indices_dst -- the batch-first order the
 * reference produces at src/models/SPConvNet.py:64 -- either destination may be NULL), feats (feat_bytes bytes),
 * labels int64 [B], and the row count n into *n_valid_dst (may be NULL).  event_offsets (may be NULL): the
 * wfs_event_offsets table of the batch (`events` events, wfs_event_offsets_ints(events) ints; the batch index is the
 * source column that perm_host moves to the front), written by the same launch -- the captured step then starts with
 * the event-local rulebook build itself. */
int wfs_load_batch(const int32_t *coords, int64_t n, int32_t cols, const int32_t *perm_host, int32_t *coords_dst,
                   int32_t *indices_dst, const void *feats, void *feats_dst, int64_t feat_bytes,
                   const int64_t *labels, int64_t *labels_dst, int64_t B, int64_t *n_valid_dst,
                   int32_t *event_offsets, int32_t events, void *stream);

/* filter images -----------------------------------------------------------------------------------------
 * The 32 -> 32 kernels for 16-bit rows (wfs_gather_conv, wfs_conv_backward) start every block by converting the layer's
 * fp32 filter into a 16-bit LDS image.  A caller whose filters change once per step can have that image made once per
 * step and hand it to those calls, whose blocks then copy it into LDS as it is.  Additions only: WFS_ABI_VERSION stays.
 *
 * An image of W [K, 32, 32] fp32 (K <= 32) for the row type `dtype` (WFS_BF16 / WFS_F16) is K * 128 fragments of 16 bytes
 * (wfs_filter_image_bytes: K * 2048 bytes; 16-byte aligned):
 *     img[k][s][h][col][j] = dtype(B[16h + 8s + j][col]),   s, h in {0, 1}, col in [0, 32), j in [0, 8),
 * with B = W[k] in the forward image (wfs_gather_conv with transpose_w == 0) and B = W[k]^T in the dX image
 * (transpose_w != 0, wfs_conv_backward), rounded as the kernels round (to nearest even).
 *
 * wfs_conv_filter_images: one launch that fills the images of one filter; either image may be NULL.
 * wfs_load_batch_images: wfs_load_batch with up to WFS_FILTER_IMAGE_JOBS_MAX image jobs in the same launch (the
 *   hand-over is the head of every captured step and reads the filters as the previous step's optimizer left them).
 *   The copy part is wfs_load_batch's, unchanged; njobs == 0 is wfs_load_batch.
 * wfs_gather_conv_image / wfs_conv_backward_image: wfs_gather_conv / wfs_conv_backward with the image of the orientation
 *   the call contracts with (forward image for transpose_w == 0, dX image otherwise); NULL = the plain entry.  The
 *   image is read only by the 32 -> 32 kernels for 16-bit rows and K <= 27; every other route ignores it.  The image
 *   must hold W's current values: the results are then bit-identical to the plain entry's. */
#define WFS_FILTER_IMAGE_JOBS_MAX 16
typedef struct wfs_filter_image_job {
    const float *W;       /* [K, 32, 32] fp32 */
    void *img_fwd;        /* K * 2048 bytes or NULL */
    void *img_t;          /* K * 2048 bytes or NULL */
    int32_t K;
    int32_t dtype;
} wfs_filter_image_job;
size_t wfs_filter_image_bytes(int32_t K);
int wfs_conv_filter_images(const float *W, int32_t K, int32_t dtype, void *img_fwd, void *img_t, void *stream);
int wfs_load_batch_images(const int32_t *coords, int64_t n, int32_t cols, const int32_t *perm_host, int32_t *coords_dst,
                          int32_t *indices_dst, const void *feats, void *feats_dst, int64_t feat_bytes,
                          const int64_t *labels, int64_t *labels_dst, int64_t B, int64_t *n_valid_dst,
                          int32_t *event_offsets, int32_t events, const wfs_filter_image_job *jobs, int32_t njobs,
                          void *stream);
/* wfs_load_rows_batch: the hand-over of a PER-ROW batch (one target row per coordinate row) in one launch.  Additions
 * only: WFS_ABI_VERSION stays.  Coordinates, permutation, row count, event offsets and image jobs are wfs_load_batch's /
 * wfs_load_batch_images' (cols 1 .. 8; the 16-byte row path for cols == 4 when all three pointers are 16-byte aligned).
 *   feats        n rows of row_bytes bytes, copied as bytes into the first n rows of feats_dst [n_cap rows]: 16-byte
 *                lanes with a byte tail when source and destination are 16-byte aligned, bytes otherwise.  Rows at and
 *                beyond n are not written.
 *   targets      n rows of target_row_bytes bytes of `elem`-byte elements (elem 4 or 8, target_row_bytes % elem == 0,
 *                pointers aligned to elem) into rows [0, n) of targets_dst; rows [n, n_cap) of targets_dst get the pad
 *                element in every position: pad_host points at 8 HOST bytes of which the first `elem` are used (the
 *                int64 ignore_index, or its float32 / float64 image).
 * n <= n_cap.  A source may be NULL when it has no bytes to give; a destination with bytes to take may not. */
int wfs_load_rows_batch(const int32_t *coords, int64_t n, int64_t n_cap, int32_t cols, const int32_t *perm_host,
                        int32_t *coords_dst, int32_t *indices_dst, const void *feats, void *feats_dst, int64_t row_bytes,
                        const void *targets, void *targets_dst, int64_t target_row_bytes, int32_t elem,
                        const void *pad_host, int64_t *n_valid_dst, int32_t *event_offsets, int32_t events,
                        const wfs_filter_image_job *jobs, int32_t njobs, void *stream);
int wfs_gather_conv_image(const int32_t *table, const int32_t *kmap_host, int32_t K, int32_t identity_k,
                          int64_t R, const void *X, int64_t X_rows, int32_t Cx, const float *W,
                          int32_t Cw_in, int32_t Cw_out, int32_t transpose_w, const float *bias, void *Y,
                          int32_t dtype, const int64_t *r_dev, int32_t packed_kl, const void *image, void *stream);
int wfs_conv_backward_image(const int32_t *table, int32_t K, int32_t identity_k, int64_t R, const void *X, const void *dY,
                            int64_t dY_rows, int32_t Cin, int32_t Cout, const float *W, void *dX, float *dW, int32_t dtype,
                            void *workspace, size_t workspace_bytes, const int64_t *r_dev, wfs_dw_job *defer,
                            int32_t packed_kl, const void *image_t, void *stream);

/* evaluation statistics (csrc/evalstats.hip) ----------------------------------------------------------
 * The per-batch work of the reference's PSDEvaluator.add (src/evaluation/PSDEvaluator.py:101-198) on the device.  These
 * entry points are additions: no existing signature or struct changes, so WFS_ABI_VERSION stays.
 *
 * wfs_event_pulse_stats (two launches: event offsets, then one workgroup per event): what average_pulse computes
 * (src/utils/SparseUtils.py:405-487).
 *   coords      int32 [n_cap, 3] = (x, y, event), rows of an event contiguous, event column non-decreasing in [0, E)
 *   rows        [n_cap, 2T] of `dtype`, left PMT first; only read.  1 <= T <= WFS_EVAL_MAX_SAMPLES
 *   n_dev       valid rows as everywhere (NULL = n_cap); rows beyond it are never read
 *   gains       double [nx, ny, 2]; seg_status float [nx, ny] (0.5 = single-ended)
 *   offsets     int32 [E + 1] scratch (first row of every event), zero-initialised once by the caller
 *   rowstats    double [n_cap, 4] scratch
 *   outputs     avg_coo double [E, 2]; summed float [E, 2T]; stats float [6, E] = x, y, dt, E spreads, time variance,
 *               sample variance; multiplicity, n_se int32 [E]; psdl, psdr, energy float [E] (energy = half the summed
 *               pulse's sum); features float [9, E] in the order of the reference's metric_names.  An event without
 *               rows gets multiplicity 0 and zeros.  n_se of event E - 1 is written as 0 unless fix_last_n_se (the
 *               reference's loop never stores it).
 *   flags       int32 [1], STICKY bits: 1 event column unsorted / out of range, 2 segment outside [nx, ny],
 *               4 (set by wfs_eval_accumulate) prediction or label outside [0, n_classes)
 * wfs_eval_accumulate (one launch): folds the batch into persistent tables.  tables int64
 *   [wfs_eval_table_ints], in this order, count table then match-sum table for the first three:
 *   mult [n_mult + 2] x 2, ene_psd [(n_bins + 2)^2] x 2 (every event twice: psdl and psdr), pos [(nx + 2)(ny + 2)] x 2,
 *   confusion_energy [n_confusion + 1, C, C], confusion_SE [n_se_max + 2, C, C] (label-major), n_wfs [C + 1],
 *   n_labelled_wfs [C].  Bin edges are the reference's: the first j with j * width + low > value in fp64.
 *   sum_wf double [C + 1, 2T] (all, then by label), sum_labelled double [C, 2T] (by prediction): += the batch's summed
 *   pulses, added in event order by one thread per element (deterministic). */
#define WFS_EVAL_MAX_SAMPLES 512
size_t wfs_eval_table_ints(int32_t n_bins, int32_t n_mult, int32_t n_confusion, int32_t n_se_max, int32_t nx,
                           int32_t ny, int32_t n_classes);
int wfs_event_pulse_stats(const int32_t *coords, const void *rows, int64_t n_cap, int32_t T, int32_t dtype,
                          const int64_t *n_dev, int32_t E, const double *gains, const float *seg_status, int32_t nx,
                          int32_t ny, int32_t fix_last_n_se, int32_t *offsets, double *rowstats, double *avg_coo,
                          float *summed, float *stats, int32_t *multiplicity, int32_t *n_se, float *psdl, float *psdr,
                          float *energy, float *features, int32_t *flags, void *stream);
int wfs_eval_accumulate(int32_t E, int32_t T, int32_t n_classes, const double *avg_coo, const float *summed,
                        const int32_t *multiplicity, const int32_t *n_se, const float *psdl, const float *psdr,
                        const float *energy, const int64_t *predictions, const int64_t *labels, int32_t n_bins,
                        int32_t n_mult, int32_t n_confusion, int32_t n_se_max, int32_t nx, int32_t ny, double emin,
                        double emax, double psd_min, double psd_max, int64_t *tables, double *sum_wf,
                        double *sum_labelled, int32_t *flags, void *stream);

/* extracted-feature evaluation statistics (csrc/physstats.hip) ---------------------------------------
 * The per-batch work of the reference's PhysEvaluator.add (src/evaluation/PSDEvaluator.py:319-397) on the device.
 * Additions only: WFS_ABI_VERSION stays.
 *
 * wfs_phys_event_stats (two launches: event offsets, then one wavefront per event): weighted_average_quantities
 * (src/utils/SparseUtils.py:490-529) over the derived columns energy = f0 * 12, psd = f5, dt = (f1 - 0.5) * 30,
 * PEL = f2 * 5000, PER = f3 * 5000, z = (f4 - 0.5) * 1200, t0 = f6 * 30, formed in fp32.
 *   coords      int32 [n_cap, 3] = (x, y, event), rows of an event contiguous, event column non-decreasing in [0, E)
 *   rows        [n_cap, 7] of `dtype`; only read.  n_dev: valid rows as everywhere (NULL = n_cap)
 *   offsets     int32 [E + 1] scratch, zero-initialised once by the caller
 *   outputs     avg_coo double [E, 2]; features float [8, E] = energy, psd, dt, PEL, PER, z, t0, multiplicity;
 *               multiplicity int32 [E].  Sums run in row order with the reference's accumulator types under numba (energy
 *               and coordinates fp64, the six weighted quantities fp32, products and sums rounded separately); the
 *               coordinate sum weighs a row by the RUNNING energy, as the reference does.  An event whose energy sum is
 *               not > 0 keeps its un-normalised sums, energy 0 and multiplicity 0; one without rows gets zeros.
 *   flags       int32 [1], STICKY bits: 1 event column unsorted / out of range, 4 (set by wfs_phys_accumulate) prediction
 *               or label outside [0, n_classes)
 * wfs_phys_accumulate (one launch): folds the batch into persistent tables.  tables int64 [wfs_phys_table_ints], count
 *   table then match-sum table each: mult [n_mult + 2], ene_psd [(n_bins + 2)^2], pos [(nx + 2)(ny + 2)]; then
 *   confusion_energy [n_confusion + 1, C, C] (label-major); then per TRUE class ene_psd_prec [C][2][(n_bins + 2)^2],
 *   ene_prec [C][2][n_bins + 2], mult_prec [C][2][n_mult + 2].  Bin edges are the reference's.
 *   spectra     NULL, or int64 [wfs_phys_spectra_ints] = [by truth | by prediction][C][8 features][bins_f + 2] in
 *               hist_add_1d's convention (underflow first, overflow last); spec_ranges HOST double [8, 2], spec_bins HOST
 *               int32 [8]. */
size_t wfs_phys_table_ints(int32_t n_bins, int32_t n_mult, int32_t n_confusion, int32_t nx, int32_t ny,
                           int32_t n_classes);
size_t wfs_phys_spectra_ints(int32_t n_classes, const int32_t *spec_bins);
int wfs_phys_event_stats(const int32_t *coords, const void *rows, int64_t n_cap, int32_t dtype, const int64_t *n_dev,
                         int32_t E, int32_t *offsets, double *avg_coo, float *features, int32_t *multiplicity,
                         int32_t *flags, void *stream);
int wfs_phys_accumulate(int32_t E, int32_t n_classes, const double *avg_coo, const float *features,
                        const int32_t *multiplicity, const int64_t *predictions, const int64_t *labels, int32_t n_bins,
                        int32_t n_mult, int32_t n_confusion, int32_t nx, int32_t ny, double emin, double emax,
                        double psd_min, double psd_max, int64_t *tables, const double *spec_ranges,
                        const int32_t *spec_bins, int64_t *spectra, int32_t *flags, void *stream);

/* per-segment evaluation tables (csrc/segstats.hip) ---------------------------------------------------
 * The per-batch work of the reference's ZEvaluatorWF.add and EnergyEvaluatorWF.add without a calibration group
 * (src/evaluation/ZEvaluator.py:528-562, EnergyEvaluator.py:132-145) on the device: the row walks z_deviation,
 * z_deviation_with_E, z_error and E_deviation of src/utils/SparseUtils.py.  Additions only: WFS_ABI_VERSION stays.
 *
 * Both entry points make two launches (event offsets, then one thread per row) on `stream` and read nothing back.
 *   coords      int32 [n_cap, 3] = (x, y, event), event column non-decreasing in [0, B); n_dev as everywhere
 *   maps        a [B, nx, ny] plane of a [B, P, nx, ny] tensor of `dtype`: element (b, x, y) of plane `plane` is
 *               base[b * bs + plane * ps + x * ny + y] (bs, ps in elements); only read.  energy may be NULL.
 *   seg_status  float [nx, ny]: > 0 = the "single" tables, else the "dual" ones
 *   sample_segs int32 [n_sample, 2] on the device (wfs_seg_z_accumulate)
 *   offsets     int32 [B + 1] scratch, zero-initialised once by the caller
 *   A row's multiplicity is the length of its event's run; its column is mult - 1 for 0 < mult <= nmult, else nmult.
 *   tables      int64, persistent.  Every (count, sum) pair is a count table followed by a sum table of the same
 *               shape; a sum cell holds the sum of round(dev * WFS_SEG_FIXED_ONE), added with integer atomics (exact,
 *               order-independent).  wfs_seg_z_table_ints, in this order: seg_mult_mae [nx, ny, nmult + 1] pair,
 *               z_mult_mae_single, z_mult_mae_dual, E_mult_mae_single, E_mult_mae_dual [nz + 2, nmult + 1] pairs,
 *               seg_sample_error [n_sample, nmult + 1, n_err + 2] counts.  wfs_seg_energy_table_ints: seg_mult_Emape
 *               [nx, ny, nmult + 1] pair, E_mult_single, E_mult_dual [nE + 2, nmult + 1] pairs.
 *   z tables    dev = |p - t|; z bin of (t - 0.5) * zrange: the first k with k * (zrange / nz) - zrange / 2 > it, 0
 *               below -zrange / 2, nz + 1 from zrange / 2; with an energy map the E bin of float(E * E_scale) is
 *               get_bin_index over [E_low, E_high) in nz bins.  Histogram: (p - t) * zrange over [err_low, err_high).
 *   energy      dev = |p - t| / t; E bin of t * E_scale over [E_low, E_high) in nE bins; a row with t == 0 is left
 *               out (flag 4).  All of it in fp64 on the fp32 value of the element, products and sums rounded apart.
 *   flags       int32 [1], STICKY bits: 1 event column unsorted / out of range, 2 segment outside [nx, ny], 4 zero
 *               energy target, 8 a deviation without a fixed-point image (not finite or |dev| >= 2^30) or a sum cell
 *               that left int64.  Rows that raise 1, 2, 4 or the first kind of 8 are left out. */
#define WFS_SEG_FIXED_ONE 4294967296.0
size_t wfs_seg_z_table_ints(int32_t nx, int32_t ny, int32_t nmult, int32_t nz, int32_t n_err, int32_t n_sample);
size_t wfs_seg_energy_table_ints(int32_t nx, int32_t ny, int32_t nmult, int32_t nE);
int wfs_seg_z_accumulate(const int32_t *coords, int64_t n_cap, const int64_t *n_dev, int32_t B, const void *pred,
                         int32_t pred_dtype, int64_t pred_bs, int64_t pred_ps, int32_t pred_plane, const void *targ,
                         int32_t targ_dtype, int64_t targ_bs, int64_t targ_ps, int32_t targ_plane, const void *energy,
                         int32_t e_dtype, int64_t e_bs, int64_t e_ps, int32_t e_plane, const float *seg_status,
                         int32_t nx, int32_t ny, const int32_t *sample_segs, int32_t n_sample, int32_t nmult,
                         int32_t nz, double zrange, int32_t n_err, double err_low, double err_high, double E_low,
                         double E_high, double E_scale, int32_t *offsets, int64_t *tables, int32_t *flags,
                         void *stream);
int wfs_seg_energy_accumulate(const int32_t *coords, int64_t n_cap, const int64_t *n_dev, int32_t B, const void *pred,
                              int32_t pred_dtype, int64_t pred_bs, int64_t pred_ps, int32_t pred_plane,
                              const void *targ, int32_t targ_dtype, int64_t targ_bs, int64_t targ_ps,
                              int32_t targ_plane, const float *seg_status, int32_t nx, int32_t ny, int32_t nmult,
                              int32_t nE, double E_low, double E_high, double E_scale, int32_t *offsets,
                              int64_t *tables, int32_t *flags, void *stream);

/* pairwise metric tables and the PID evaluator's rows (csrc/metricpairs.hip) -----------------------------
 * The reference's MetricPairAggregator (src/evaluation/MetricAggregator.py:339-366) and the per-row half of
 * PIDEvaluator.add (src/evaluation/PIDEvaluator.py:93-135) on the device.  Additions only: WFS_ABI_VERSION stays.
 *
 * wfs_metric_pairs_accumulate (one launch on `stream`, no read-back): bins a 0/1 result of M elements by each of P
 * parameters and by every pair of them, per category.
 *   params      float [P, M], row-major; 1 <= P <= WFS_METRIC_PAIRS_MAX; only read
 *   result      int32 [M], 0 or 1 (anything else: flag 8, element left out)
 *   category    int32 [M] in [0, n_classes); -1 = the element is skipped; anything else: flag 4, element left out
 *   n_dev       valid elements as everywhere (NULL = M); elements beyond it are never read
 *   lo, hi      double [P] on the HOST, hi > lo; nbins int32 [P] on the host, >= 1
 *   tables      int64 [wfs_metric_pairs_table_ints], persistent, in this order: for each metric i a count table
 *               [n_classes, nbins[i] + 2], then its match-sum table of the same shape; then for each pair i < j in the
 *               order 0_1, 0_2, .., 0_P-1, 1_2, .. a count table [n_classes, nbins[i] + 2, nbins[j] + 2], then its
 *               match-sum table.  Integer atomics only: exact, order-independent.
 *   bins        get_bin_index in fp64 on the fp32 value: 0 below lo, nbins + 1 from hi, else the first j in 1 .. nbins
 *               with j * ((hi - lo) / nbins) + lo > value (rounded product, rounded sum); 0 if there is none (NaN, or
 *               a value just below hi that no rounded edge exceeds).  Computed without walking the bins.
 *   flags       int32 [1], STICKY bits: 4 category outside [-1, n_classes), 8 result not 0 / 1
 * wfs_match_categories (one launch): result[m] = (predictions[m] == labels[m]), category[m] = labels[m] (a label
 *   outside int32 becomes -2, which the accumulate flags), for a caller that holds int64 class indices [M].
 * wfs_pid_row_stats (two launches: event offsets, then one thread per row):
 *   coords      int32 [n_cap, 3] = (x, y, event), event column non-decreasing in [0, E); n_dev as everywhere
 *   predictions, targets  int64 [n_cap] in [0, WFS_PID_CLASSES)
 *   phys        [n_cap, n_phys] of `dtype`; columns e_index, psd_index, z_index are read
 *   seg_status  float [nx, ny] (0.5 = single-ended); offsets int32 [E + 1] scratch, zero-initialised once
 *   outputs     per row, int32 [n_cap]: accuracy (prediction == target), multiplicity (rows of the row's event, the
 *               lookahead ends with the valid rows), se (seg_status == 0.5), n_se (single-ended rows of the row's
 *               event), category (target if se else -1); params float [4, n_cap] = E, PSD, multiplicity, z.  Rows
 *               beyond the valid count and flagged rows get zeros and category -1.
 *   tables      int64 [wfs_pid_table_ints], persistent, label-major [.., target, prediction]: SE_confusion [5, 5] over
 *               single-ended rows, confusion_SE [n_se_max + 2, 5, 5] by n_se over [-0.5, n_se_max + 0.5] in
 *               n_se_max + 1 bins, confusion_energy [n_confusion + 1, 5, 5] by E over [0, e_high] in n_confusion bins;
 *               both with confusion_accumulate_1d's edges (a value above the range is dropped, one at it is bin 0).
 *   flags       int32 [1], STICKY bits: 1 event column unsorted / out of range, 2 segment outside [nx, ny],
 *               4 prediction or target outside [0, WFS_PID_CLASSES).  Flagged rows are left out. */
#define WFS_METRIC_PAIRS_MAX 16
#define WFS_PID_CLASSES 5
size_t wfs_metric_pairs_table_ints(int32_t P, const int32_t *nbins, int32_t n_classes);
int wfs_metric_pairs_accumulate(const float *params, const int32_t *result, const int32_t *category, int64_t M,
                                const int64_t *n_dev, int32_t P, const double *lo, const double *hi,
                                const int32_t *nbins, int32_t n_classes, int64_t *tables, int32_t *flags, void *stream);
int wfs_match_categories(const int64_t *predictions, const int64_t *labels, int64_t M, int32_t *result,
                         int32_t *category, void *stream);
size_t wfs_pid_table_ints(int32_t n_confusion, int32_t n_se_max);
int wfs_pid_row_stats(const int32_t *coords, const int64_t *predictions, const int64_t *targets, const void *phys,
                      int32_t n_phys, int32_t dtype, int64_t n_cap, const int64_t *n_dev, int32_t E,
                      const float *seg_status, int32_t nx, int32_t ny, int32_t e_index, int32_t psd_index,
                      int32_t z_index, int32_t n_confusion, int32_t n_se_max, double e_high, int32_t *offsets,
                      int32_t *accuracy, int32_t *multiplicity, int32_t *se, int32_t *n_se, float *params,
                      int32_t *category, int64_t *tables, int32_t *flags, void *stream);

/* real-valued metric tables and the TensorEvaluator's rows (csrc/metricpairs.hip) ------------------------
 * The reference's TensorEvaluator.add (src/evaluation/TensorEvaluator.py:70-91) on the device: a per-row LOSS binned by
 * each of P parameters and by every pair of them, and summed per PMT.  Additions only: WFS_ABI_VERSION stays.
 *
 * wfs_metric_pairs_accumulate_real (one launch on `stream`, no read-back): as wfs_metric_pairs_accumulate, for a result
 * that is a real number.
 *   result      float [M]; its fixed-point image is v = round(result * 2^32).  A result without an image (not finite, or
 *               |result| >= 2^15): flag 8, element left out
 *   params, category, n_dev, lo, hi, nbins, bins   as wfs_metric_pairs_accumulate
 *   tables      int64 [wfs_metric_pairs_real_table_ints], persistent, in this order: for each metric i FIVE tables
 *               [n_classes, nbins[i] + 2]: the count n, S = sum v, and Q0, Q1, Q2 with sum v^2 = Q0 + Q1 2^32 + Q2 2^64
 *               (the sums of the three 32-bit pieces of every v^2 < 2^94: each fits an int64 for 2^31 elements per
 *               cell); then for each pair i < j in the order 0_1, 0_2, .., 1_2, .. a count table
 *               [n_classes, nbins[i] + 2, nbins[j] + 2], then its S table.  Integer atomics only: exact, independent of
 *               the order of the elements and of the launch shape, N ranks combine them with one integer SUM.  The host
 *               forms mean = S / (n 2^32) and M2 = (n Q - S^2) / (n 2^64) from the integers.
 *   flags       int32 [1], STICKY bits: 4 category outside [-1, n_classes), 8 result without a fixed-point image,
 *               16 a cell's S left int64
 * wfs_tensor_rows (one launch, one thread per row):
 *   c           detector numbers [N] (c_cols = 1) or (x, y, side) rows [N, 3] (c_cols = 3); int32, or int64 with c_int64
 *   target      [N, P] of target_dtype (WFS_F32 / WFS_BF16 / WFS_F16, or WFS_TENSOR_TARGET_I64 for class indices);
 *               1 <= P <= WFS_METRIC_PAIRS_MAX, P = 1 for a target [N]
 *   results     float [N], the per-row loss; n_dev as everywhere, rows beyond it are never read
 *   outputs     params float [P, N] (the transposed target), category int32 [N]: 0, or -1 beyond the valid rows (whose
 *               params are 0)
 *   det_tables  int64 [2 * nx * ny * 2], persistent: the count table [nx, ny, 2], then the table of sum v.  A detector
 *               number decodes as the reference compares it, det == 2 * (14 * y + x) + side (nx <= 14); a row whose PMT
 *               lies outside the grid is left out of these tables only.
 *   flags       int32 [1], STICKY bits 8 and 16 as above (such a row is left out of det_tables) */
#define WFS_TENSOR_TARGET_I64 3
size_t wfs_metric_pairs_real_table_ints(int32_t P, const int32_t *nbins, int32_t n_classes);
int wfs_metric_pairs_accumulate_real(const float *params, const float *result, const int32_t *category, int64_t M,
                                     const int64_t *n_dev, int32_t P, const double *lo, const double *hi,
                                     const int32_t *nbins, int32_t n_classes, int64_t *tables, int32_t *flags,
                                     void *stream);
int wfs_tensor_rows(const void *c, int32_t c_int64, int32_t c_cols, const void *target, int32_t target_dtype, int32_t P,
                    const float *results, int64_t N, const int64_t *n_dev, int32_t nx, int32_t ny, float *params,
                    int32_t *category, int64_t *det_tables, int32_t *flags, void *stream);

/* the per-segment regression module: masked loss (csrc/segloss.hip) and the SegEvaluator's rows (csrc/segquant.hip)
 * Additions only: WFS_ABI_VERSION stays.
 *
 * wfs_masked_regression_loss (ONE launch on `stream`): the mean of |d| (WFS_LOSS_L1) or d^2 (WFS_LOSS_MSE),
 * d = pred - target[:, col], over the COUNTED rows: those below the valid count and, with a mask, on a segment whose mask
 * entry is 1.0.  A row that is not counted is selected out: nothing in it (NaN, Inf, padding) reaches a result.
 *   pred        [n_cap] of pred_dtype; target [n_cap, n_cols] of target_dtype (n_cols = 1, col = 0 for a target [n_cap])
 *   coords      int32 [n_cap, 3] = (x, y, event), read only with a mask; se_mask float [nx, ny] or NULL
 *   n_dev       as everywhere; max_blocks 0 = the default grid (the result does not depend on it)
 *   workspace   wfs_masked_regression_loss_workspace_bytes(n_cap) bytes whose first 4 are ZERO before the first use; the
 *               launch leaves them zero, so a buffer is zeroed once.  One launch at a time per workspace.
 *   out         float [2]: the loss and the mean of d^2 over the same rows; count int64 [1].  d and all sums are fp64,
 *               chunk sums are folded in a fixed order, no floating-point atomics: bit-identical from run to run and
 *               independent of the grid.  No row counted: NaN, NaN, 0.
 * wfs_masked_regression_loss_backward (ONE launch): dpred [n_cap] of pred_dtype = grad[0] * s / count[0] with
 *   s = sign(d) (sign(0) = 0) for L1, 2 d for MSE; exactly 0 in a row that is not counted, and everywhere when count is 0.
 *
 * wfs_error_edges (host only): first_last[0 .. 1] = the first and last entry of the reference's
 *   get_bins(-1.1 max_abs, 1.1 max_abs, n_bins) = np.arange(low, high + w / 2, w), bit for bit; WFS_EINVAL for a
 *   max_abs that is 0, negative or not finite.  The device fixes the ErrorAggregator's ranges with the same function.
 * wfs_segq_row_stats (two launches: event offsets, then one thread per row), SegEvaluator.add's row walks:
 *   results     [n_cap] of results_dtype; target [n_cap, n_phys] of target_dtype; pid int32 / int64 [n_cap] or NULL
 *   outputs     per row: mae float = |error|, error double = results - target[:, target_index] in fp64, multiplicity,
 *               se (seg_status == 0.5), category, slot (int32), params float [4, n_cap] = E, PSD, multiplicity, z.
 *               With pid: slot = the PID's place in 1 | 4 | 6, 258 | 256 | 512 and category = its class 0 .. 4 on a
 *               valid single-ended row whose PID is in that list, else both -1.  Without: slot = category = 0 for every
 *               valid row.  Rows beyond the valid count and flagged rows get zeros and -1.
 *   slot_scratch int64 [2 * 6], zero before the first use: per slot max |error| (the bits of the double) and the row
 *               count of this batch; wfs_segq_error_accumulate consumes and clears them.
 *   flags       int32 [1], STICKY bits: 1 event column unsorted / out of range, 2 segment outside [nx, ny]
 * wfs_segq_error_accumulate (two launches: one workgroup fixing edges, then one thread per row), ErrorAggregator.add_norm:
 *   n_classes is 5 with has_pid, 1 without.  edges double [n_classes, 2], edges_set int32 [n_classes], persistent: a class that is not set takes the first slot
 *   with rows in this batch; error_flags int32 [1], STICKY bit c: class c's first subset had a max |error| of 0 or not
 *   finite (its edges stay unset and its rows are not binned).  error_hist int64 [n_classes, n_bins + 2] by the class's
 *   edges, error_2d int64 [n_classes, n_bins + 2, n_bins + 2] by (actual, predicted) over [0, 1]. */
#define WFS_LOSS_L1 0
#define WFS_LOSS_MSE 1
size_t wfs_masked_regression_loss_workspace_bytes(int64_t n_cap);
int wfs_masked_regression_loss(const void *pred, int32_t pred_dtype, const void *target, int32_t target_dtype,
                               int32_t n_cols, int32_t col, const int32_t *coords, const float *se_mask, int32_t nx,
                               int32_t ny, int64_t n_cap, const int64_t *n_dev, int32_t kind, int32_t max_blocks,
                               void *workspace, size_t workspace_bytes, float *out, int64_t *count, void *stream);
int wfs_masked_regression_loss_backward(const void *pred, int32_t pred_dtype, const void *target, int32_t target_dtype,
                                        int32_t n_cols, int32_t col, const int32_t *coords, const float *se_mask,
                                        int32_t nx, int32_t ny, int64_t n_cap, const int64_t *n_dev, int32_t kind,
                                        const int64_t *count, const float *grad, void *dpred, void *stream);
int wfs_error_edges(double max_abs, int32_t n_bins, double *first_last);

/* the segment loss of the dense-map regression modules, LitZ / LitEZ (csrc/segloss.hip) ---------------------
 * Additions only: WFS_ABI_VERSION stays.
 *
 * wfs_segment_map_loss (ONE launch on `stream`): the reference's LitBase._calc_segment_loss for up to 4 planes at once.
 * A row is COUNTED when it lies below the valid count, its (x, y, event) lies inside [nx, ny, B] and, with a mask, its
 * mask entry is 1.0.  For a counted row and plane p, d = map[event, p, x, y] - target[row, cols[p]] in fp64.  A row that
 * is not counted is selected out: nothing in it, and no map cell outside the counted rows, reaches a result;
 * coordinates beyond the valid count are never read.
 *   map         [B, planes, nx, ny] of map_dtype, planes <= 4, nx * ny <= 256; coords int32 [n_cap, 3] = (x, y, event)
 *   target      [n_cap, n_cols] of target_dtype; cols HOST int32 [planes]: plane p is scored against column cols[p]
 *   se_mask     float [nx, ny] or NULL; n_dev as everywhere; kind WFS_LOSS_L1 / WFS_LOSS_MSE
 *   max_blocks  0 = the default grid (the result does not depend on it)
 *   workspace   wfs_segment_map_loss_workspace_bytes(n_cap, planes) bytes whose first 4 are ZERO before the first use;
 *               the launch leaves them zero, so a buffer is zeroed once.  One launch at a time per workspace.
 *   out         float [planes + 1]: out[p] = the sum over the counted rows of |d| or d^2, divided by the count;
 *               out[planes] = the sum of those per-plane values, formed in fp64 and rounded once.  count int64 [1].
 *               fp64 chunk sums folded in a fixed order, no floating-point atomics: bit-identical from run to run and
 *               independent of max_blocks, n_cap and B.  No row counted: NaN everywhere and a count of 0.
 * wfs_segment_map_loss_backward (ONE launch) writes ALL of dmap [B, planes, nx, ny] of map_dtype (16-byte aligned):
 *   grad[0] * s / count[0] at a counted row's cell, s = sign(d) (sign(0) = 0) for L1, 2 d for MSE, and exactly 0 in
 *   every other cell -- events without rows and events beyond the batch's own included -- and everywhere when count is 0.
 *   The rows of the batch are grouped by event in ascending order (as for the rulebook builds).  Segments are unique
 *   within an event; where one is duplicated each row counts in the forward and the cell gets the sum of its rows'
 *   values in row order. */
size_t wfs_segment_map_loss_workspace_bytes(int64_t n_cap, int32_t planes);
int wfs_segment_map_loss(const void *map, int32_t map_dtype, int64_t B, int32_t planes, int32_t nx, int32_t ny,
                         const int32_t *coords, const void *target, int32_t target_dtype, int32_t n_cols,
                         const int32_t *cols, const float *se_mask, int64_t n_cap, const int64_t *n_dev, int32_t kind,
                         int32_t max_blocks, void *workspace, size_t workspace_bytes, float *out, int64_t *count,
                         void *stream);
int wfs_segment_map_loss_backward(const void *map, int32_t map_dtype, int64_t B, int32_t planes, int32_t nx, int32_t ny,
                                  const int32_t *coords, const void *target, int32_t target_dtype, int32_t n_cols,
                                  const int32_t *cols, const float *se_mask, int64_t n_cap, const int64_t *n_dev,
                                  int32_t kind, const int64_t *count, const float *grad, void *dmap, void *stream);
int wfs_segq_row_stats(const int32_t *coords, const void *results, int32_t results_dtype, const void *target,
                       int32_t target_dtype, int32_t n_phys, const void *pid, int32_t pid_int64, int64_t n_cap,
                       const int64_t *n_dev, int32_t E, const float *seg_status, int32_t nx, int32_t ny, int32_t e_index,
                       int32_t psd_index, int32_t z_index, int32_t target_index, int32_t *offsets, float *mae,
                       double *error, int32_t *multiplicity, int32_t *se, float *params, int32_t *category,
                       int32_t *slot, int64_t *slot_scratch, int32_t *flags, void *stream);
int wfs_segq_error_accumulate(const void *results, int32_t results_dtype, const void *target, int32_t target_dtype,
                              int32_t n_phys, int32_t target_index, const double *error, const int32_t *category,
                              int64_t n_cap, const int64_t *n_dev, int32_t n_classes, int32_t has_pid, int32_t n_bins,
                              int64_t *slot_scratch, double *edges, int32_t *edges_set, int32_t *error_flags,
                              int64_t *error_hist, int64_t *error_2d, void *stream);

/* the real-data z evaluator (csrc/zreal.hip) --------------------------------------------------------------
 * The reference's ZEvaluatorRealWFNorm.add (src/evaluation/ZEvaluator.py:620-670, with WaveformEvaluator.analyze_wf_z and
 * RealDataEvaluator.add) on the device.  Additions only: WFS_ABI_VERSION stays.  Raw pointers, an explicit stream, the
 * valid row count in device memory (n_dev, NULL = all), STICKY flags, no read-back, integer atomics only.
 *
 * wfs_align_pulses (one launch, one wavefront per row): align_wfs(n_before = 1) of src/utils/WaveformUtils.py.
 *   feats       [n_cap, 2 L] of dtype: the left PMT's L samples, then the right PMT's; 1 <= L <= 512
 *   samples     float [2, P, n_cap] (side, sample, row): the params of wfs_metric_pairs_accumulate_real per side;
 *               1 <= P <= 16.  Sample k of a side is row[k + start]; samples before the row's start or beyond its end are
 *               0 (the reference indexes past the row for a peak in the last samples)
 *   start       int32 [n_cap, 2] = round_half_even(peak + tx) - 1 per side, -1 where the pulse starts at sample 0.
 *               find_peak: the plateau-centred local maxima, the first one strictly above the running best, index 0 if
 *               none beats sample 0; calc_crossing(-0.5): down the rising edge to half height, linear interpolation, 0
 *               where the result leaves the row.  fp64 arithmetic on the stored values.  Rows beyond the valid count:
 *               zeros, never read.
 * wfs_zreal_row_stats (two launches: event offsets, then one thread per row):
 *   pred, targ  dense maps [B, P, nx, ny] given as base, dtype, batch stride, plane stride (in elements) and plane
 *               indices: the prediction plane, and the target's z, energy and PSD planes
 *   pid         int32 / int64 [n_cap] or NULL; mapped 1 | 4 | 6, 258 | 256 | 512 -> 0 | 1 | 2 | 3 | 4, any other value
 *               stays as it is; without pid every row is class 0
 *   outputs     per row: z_pred, z_true, energy (the maps' elements, widened), mae = |pred - z| in fp64 (0 where the
 *               target is exactly 0), dev_mm = |(z - 0.5) z_scale - (pred - 0.5) z_scale|, se (seg_status == 0.5),
 *               params float [4, n_cap] = E, PSD, the number of single-ended rows of the row's event, z;
 *               class_category = the class on a single-ended row with pid whose class lies in [0, n_classes), else -1;
 *               sample_category = slice * n_classes + class with the z slice of analyze_wf_z (12 slices of z in mm:
 *               <= -600 | nine of 120 mm, open below | (480, 600) | >= 600), and 12 * n_classes for a valid row in no
 *               (slice, class) cell.  Rows beyond the valid count and flagged rows: zeros and -1.
 *   flags       int32 [1], STICKY: 1 event column unsorted / out of range, 2 segment outside [nx, ny], 4 a single-ended
 *               row's class index outside [0, n_classes) (left out of the class tables)
 * wfs_zreal_baseline (one launch, one lane per event, after wfs_zreal_row_stats' offsets): z_basic_prediction_dense
 *   (truth_is_cal = True) on the map that is 0.5 on single-ended segments and z_true elsewhere, per row: a row at 0.5
 *   becomes the mean of the rows of its event on the four DIAGONAL neighbour segments that are not 0.5, rows ahead first,
 *   then rows behind down to row 1 of the batch (row 0 is never a source), an fp64 sum stored once to fp32.  In place and
 *   in row order: an averaged row feeds later rows.  Segments are taken to be unique within an event.
 * wfs_zreal_accumulate (one launch, one thread per row, after the same offsets): z_deviation_with_E_full_correlation.
 *   pred_rows   float [n_cap]: z_pred, or the baseline
 *   tables      int64 [wfs_zreal_table_ints], persistent, (count table, then sum table of round(dev * WFS_SEG_FIXED_ONE))
 *               for seg_mult_zmae [nx, ny, n_mult + 1], z_mult_single, z_mult_dual [n_z + 2, n_mult + 1], z_E_single,
 *               z_E_dual [n_z + 2, n_E + 2], E_mult_single, E_mult_dual [n_E + 2, n_mult + 1], in this order.  A
 *               single-ended segment bins 588 -/+ true z by blind_left; a double-ended one is entered at both distances;
 *               a dead one (status 1) only enters E_mult_*; "single" is status > 0.
 *   flags       STICKY: 1, 2 as above, 8 a deviation without a fixed-point image (NaN: the row is left out) */
int wfs_align_pulses(const void *feats, int32_t dtype, int64_t n_cap, const int64_t *n_dev, int32_t L, int32_t P,
                     float *samples, int32_t *start, void *stream);
int wfs_zreal_row_stats(const int32_t *coords, const void *pred, int32_t pred_dtype, int64_t pred_bs, int64_t pred_ps,
                        int32_t pred_plane, const void *targ, int32_t targ_dtype, int64_t targ_bs, int64_t targ_ps,
                        int32_t z_plane, int32_t e_plane, int32_t psd_plane, const void *pid, int32_t pid_int64,
                        int64_t n_cap, const int64_t *n_dev, int32_t B, const float *seg_status, int32_t nx, int32_t ny,
                        int32_t n_classes, double z_scale, int32_t *offsets, float *z_pred, float *z_true, float *energy,
                        float *mae, float *dev_mm, float *params, int32_t *class_category, int32_t *sample_category,
                        int32_t *se, int32_t *flags, void *stream);
int wfs_zreal_baseline(const int32_t *coords, int64_t n_cap, const int64_t *n_dev, int32_t B, const int32_t *offsets,
                       const float *z_true, const float *seg_status, int32_t nx, int32_t ny, float *baseline,
                       void *stream);
size_t wfs_zreal_table_ints(int32_t nx, int32_t ny, int32_t n_mult, int32_t n_z, int32_t n_E);
int wfs_zreal_accumulate(const int32_t *coords, int64_t n_cap, const int64_t *n_dev, int32_t B, const int32_t *offsets,
                         const float *pred_rows, const float *z_true, const float *energy, const float *seg_status,
                         const int32_t *blind_left, int32_t nx, int32_t ny, int32_t n_mult, int32_t n_z, double zrange,
                         double E_low, double E_high, int32_t n_E, int64_t *tables, int32_t *flags, void *stream);

/* the calibrated z / E baseline (csrc/calibz.hip, csrc/segstats.hip) -------------------------------------
 * The reference's classical reconstruction calc_calib_z_E (src/utils/SparseUtils.py:938-1026 and its helpers :532-935)
 * and the `hascal` branches of ZEvaluatorWF.add / z_from_cal (src/evaluation/ZEvaluator.py:502-562) and
 * EnergyEvaluatorWF.add / calc_deviation_with_z (EnergyEvaluator.py:53-69,132-138) on the device.  Additions only:
 * WFS_ABI_VERSION stays.  Raw pointers, an explicit stream, n_dev as everywhere, STICKY flags, no read-back.
 *
 * wfs_calib_z_E (one launch, one wavefront per row):
 *   feats       [n_cap, 2 L] of dtype: the left PMT's L samples, then the right PMT's; 2 <= L <= WFS_CALIB_MAX_L
 *   coords      int32 [n_cap, 3] = (x, y, event); only x and y are used (they choose the segment's curves)
 *   curves      fp64 on the device, what a Calibrator carries: gain_factor = MAX_RANGE / gains, eres, sampletime
 *               [nx, ny, 2]; rel_times [nx, ny]; t_interp_curves [nx, ny, 2, WFS_CALIB_T_POINTS, 2]; time_pos_curves
 *               [nx, ny, WFS_CALIB_TIME_POINTS, 2]; light_pos_curves [nx, ny, WFS_CALIB_LIGHT_POINTS, 2];
 *               light_sum_curves [nx, ny, WFS_CALIB_SUM_POINTS, 2]; a curve is (x, y) points; a PMT whose t_interp curve has
 *               abscissa 0 at point 10 has none
 *   z_cal,E_cal double [n_cap]: z / z_scale + 0.5 and E of the row's segment, 0 where the reference leaves its map alone
 *   state       int32 [n_cap]: 0 skipped (no peak on either side), 1 one side only (z = 0.5), 2 equal peak counts
 *               (peak_to_z per pair), 3 unequal counts (match_peaks, peak_to_dt, z_dt_to_z)
 *   peaks       int32 [n_cap, 2, WFS_CALIB_PEAKS]: per side the peaks that survive cull_peaks in find_peaks' order, -1
 *               behind them.  A side with all WFS_CALIB_PEAKS slots taken counts as having no peak, as in the reference.
 *   flags       int32 [1], STICKY: 2 segment outside [nx, ny] (row skipped, state 0), 16 a row with a sample, z or E that
 *               is not finite (numba raises on the zero divisors): z_cal and E_cal hold the values as they came out (NaN for a
 *               bad sample) and the accumulate calls below leave the row out of every table.
 *   fp64 arithmetic on the stored values, rounded products and sums (no fma).  Rows beyond the valid count: zeros, -1.
 *
 * wfs_seg_z_accumulate_cal (two launches, as wfs_seg_z_accumulate): per row z_deviation_with_E + z_error twice, the
 *   prediction plane into the first table set and z_cal into a second set of the same layout behind it (the reference's
 *   `*_cal` entries): tables int64 [2 * wfs_seg_z_table_ints].  The energy axis of both: float(E * E_scale) of the energy
 *   plane when one is given, else E_cal unscaled.  target_is_cal != 0 (two more launches, row_scratch float
 *   [2, n_cap]): the second set scores, in place of z_cal, the map z_from_cal builds -- 0.5 on single-ended segments, the
 *   target elsewhere, through z_basic_prediction_dense(truth_is_cal = True), i.e. wfs_zreal_baseline on the target's rows.
 * wfs_seg_energy_accumulate_cal: E_deviation_with_z twice, the prediction plane and float(E_cal), both binned by
 *   (float(z_cal) - 0.5) * zrange over [-zrange / 2, zrange / 2) in nE bins of zrange / nE (the reference's width) into
 *   [nE + 2, nz + 2] tables, nz >= nE.  tables int64 [wfs_seg_energy_cal_table_ints]: seg_mult_Emape, E_mult_single,
 *   E_mult_dual (as wfs_seg_energy_table_ints), E_z_single, E_z_dual pairs, then the same five again for `*_cal`. */
#define WFS_CALIB_MAX_L 512
#define WFS_CALIB_PEAKS 5
#define WFS_CALIB_T_POINTS 50
#define WFS_CALIB_TIME_POINTS 50
#define WFS_CALIB_LIGHT_POINTS 51
#define WFS_CALIB_SUM_POINTS 50
int wfs_calib_z_E(const void *feats, int32_t dtype, const int32_t *coords, int64_t n_cap, const int64_t *n_dev, int32_t L,
                  int32_t nx, int32_t ny, const double *gain_factor, const double *eres, const double *rel_times,
                  const double *sampletime, const double *t_interp_curves, const double *time_pos_curves,
                  const double *light_pos_curves, const double *light_sum_curves, int32_t sample_width, double z_scale,
                  double *z_cal, double *E_cal, int32_t *state, int32_t *peaks, int32_t *flags, void *stream);
int wfs_seg_z_accumulate_cal(const int32_t *coords, int64_t n_cap, const int64_t *n_dev, int32_t B, const void *pred,
                             int32_t pred_dtype, int64_t pred_bs, int64_t pred_ps, int32_t pred_plane, const void *targ,
                             int32_t targ_dtype, int64_t targ_bs, int64_t targ_ps, int32_t targ_plane, const void *energy,
                             int32_t e_dtype, int64_t e_bs, int64_t e_ps, int32_t e_plane, const double *z_cal,
                             const double *E_cal, int32_t target_is_cal, float *row_scratch, const float *seg_status,
                             int32_t nx, int32_t ny, const int32_t *sample_segs, int32_t n_sample, int32_t nmult, int32_t nz, double zrange,
                             int32_t n_err, double err_low, double err_high, double E_low, double E_high, double E_scale,
                             int32_t *offsets, int64_t *tables, int32_t *flags, void *stream);
size_t wfs_seg_energy_cal_table_ints(int32_t nx, int32_t ny, int32_t nmult, int32_t nE, int32_t nz);
int wfs_seg_energy_accumulate_cal(const int32_t *coords, int64_t n_cap, const int64_t *n_dev, int32_t B, const void *pred,
                                  int32_t pred_dtype, int64_t pred_bs, int64_t pred_ps, int32_t pred_plane,
                                  const void *targ, int32_t targ_dtype, int64_t targ_bs, int64_t targ_ps,
                                  int32_t targ_plane, const double *z_cal, const double *E_cal, const float *seg_status,
                                  int32_t nx, int32_t ny, int32_t nmult, int32_t nE, int32_t nz, double E_low,
                                  double E_high, double E_scale, double zrange, int32_t *offsets, int64_t *tables,
                                  int32_t *flags, void *stream);

/* ---- prediction writers (csrc/predwrite.hip; reference src/datasets/PredictionWriter.py swap_values) ----------------
 * A chunk of a table travels as RAW compound records uint8 [N, item_size] (include/wfh5w.h); the two entry points turn
 * them into the net's input and put the net's output back into them, on the device.
 *
 * wfs_predict_prepare (reference normalize_waveforms, src/utils/SparseUtils.py:1564-1583), three launches:
 *   coords    int32 [cap, 3] (x, y, event): the member at coord_offset, its event column renumbered from 0, +1 wherever a
 *             row's event number differs from the previous row's (changes, not distinct values; row 0 starts event 0).
 *             Integer block sums + an in-block scan: deterministic, no atomics.
 *   feats     [cap, width] rows of feat_dtype (WFS_F32 / BF16 / F16) from the member at feat_offset:
 *             WFS_PREDICT_WAVEFORM  int16 [width]: wf[i, j] * gain_factors[x, y, j >= width / 2] in fp64 (gain_factors
 *                                   double [nx, ny, 2]), rounded once to fp32 and once more for 16-bit rows; a row whose
 *                                   (x, y) lies outside [0, nx) x [0, ny) gets NaN instead of an out-of-bounds read
 *             WFS_PREDICT_PULSE     float32 [width]: copied (rounded once for 16-bit rows)
 *   rows [N, cap): zero features, zero coordinates (what the captured runners' buffers hold there); n_valid[0] = N.
 *   Records need only be 2-byte friendly: 4-byte loads are used when item_size and the member's offset are multiples of
 *   4, 2-byte loads otherwise, decided per call.  width must be even; `records` 4-byte aligned.
 *   workspace: int32 [wfs_predict_workspace_ints(N)].
 *
 * wfs_predict_scatter (reference swap_sparse_from_dense / swap_sparse_from_event, :1459-1499): float32 columns
 *   [col0, col0 + L) of the member at member_offset of every record, in place, from
 *     WFS_PREDICT_DENSE  src [B, L, nx, ny]: row i takes src[event(i), l, x(i), y(i)]
 *     WFS_PREDICT_EVENT  src [B, L]:         row i takes src[event(i), l]
 *     WFS_PREDICT_ROWS   src [>= N, L]:      row i takes src[i, l]
 *   (x, y, event) are the PREPARED coordinates int32 [N, 3]; a row whose coordinates fall outside src is left as it is.
 *   src is fp32 / bf16 / fp16, widened exactly; affine != 0: (v - sub) * mul as an fp32 subtraction and an fp32
 *   multiplication, each rounded once, never fused.  No other byte of a record is written; no atomics; one launch. */
#define WFS_PREDICT_ROWS_PER_BLOCK 256   /* rows per workgroup of the coordinate scan */
#define WFS_PREDICT_WAVEFORM 0
#define WFS_PREDICT_PULSE 1
#define WFS_PREDICT_DENSE 0
#define WFS_PREDICT_EVENT 1
#define WFS_PREDICT_ROWS 2
size_t wfs_predict_workspace_ints(int64_t n);
int wfs_predict_prepare(const void *records, int64_t n, int64_t item_size, int64_t coord_offset, int64_t feat_offset,
                        int32_t feat_kind, int32_t width, const double *gain_factors, int32_t nx, int32_t ny, int64_t cap,
                        int32_t *coords, void *feats, int32_t feat_dtype, int64_t *n_valid, int32_t *workspace,
                        size_t workspace_ints, void *stream);
int wfs_predict_scatter(void *records, int64_t n, int64_t item_size, int64_t member_offset, int32_t member_cols,
                        int32_t col0, int32_t L, const int32_t *coords, const void *src, int32_t src_dtype, int32_t mode,
                        int64_t B, int32_t nx, int32_t ny, int32_t affine, float sub, float mul, void *stream);

/* ---- GraphNet: FiLM message passing on an event-local kNN graph (csrc/graphconv.hip) ----------------------------
 * The slice of the reference's src/models/GraphNet.py that its example configs use (graph_class_index 11): torch_cluster's
 * knn_graph and torch_geometric's FiLMConv with mean aggregation, both RESTATED (neither library is available to hold the
 * kernels to: parity unpinned).  Additions only: WFS_ABI_VERSION stays.
 *
 * Neighbour tables.  coords int32 [n_cap, 3] = (x, y, event), rows grouped by event; k in 1 .. wfs_graph_kmax() (= 8).
 *   nbr int32 [n_cap, 8]: row i's neighbours ordered by (squared integer distance on (x, y), row index), -1 padded;
 *   deg int32 [n_cap].  Candidates are the other valid rows of the same event; among equal distances the LOWER ROW INDEX
 *   wins; the row itself is left out by index (self_loop != 0: it is a candidate at distance 0 and k counts it).  CONTRACT: an
 *   event's run is at most 1024 rows (a detector event has at most 154); a row looks no further to either side, so a longer
 *   run costs bounded time and no access leaves the arrays, but its lists and reverse lists are then undefined.
 *   rev_pos int32 [n_cap, 2] = (start, count) into rev_rows int32 [n_cap * 8]: the rows that name row j as a neighbour, in
 *   ascending row order (the backward pass's fixed summation order).  Rows at and beyond the valid count get deg 0, a list
 *   of -1 and an empty reverse list, and appear in nobody's list.
 *   wfs_graph_knn: two launches (lists, reverse lists).  wfs_graph_knn_host: the same selection rule -- one
 *   __host__ __device__ function -- over HOST arrays (nbr, deg only), so that the rule can be checked without a GPU.
 * Messages.  P [n_cap, 6 D] of `dtype` holds the six column blocks s | bs | gs | h | b | g of one product row
 *   (x . lin_skip^T | split(x . film_skip^T) | x . lins.0^T | split(x . films.0^T + bias), beta first):
 *     out_i = relu(gs_i * s_i + bs_i) + (1 / deg_i) sum_{j in nbr(i)} relu(g_i * h_j + b_i)        (0 edges: first term only)
 *   wfs_film_message_fwd (one launch): out [n_cap, D] of `dtype`; rows at and beyond the valid count are written as 0.
 *   wfs_film_message_bwd (one launch): dP [n_cap, 6 D] from dout [n_cap, D]; a ReLU passes where its argument -- the same
 *   fused multiply-add of the same stored values -- is > 0; fp32 accumulators, the source-side sum walks the reverse list
 *   in its order, no atomics: bit-identical from run to run.  Rows at and beyond the valid count are not written.
 * wfs_rows_zero_tail (one launch; none without n_dev): X[n_valid .. n_cap) := 0 in place.
 * Event max (torch_geometric's global_max_pool over the event column, whose numbers ascend with the rows):
 *   wfs_event_max_fwd: Y [B, D] = the largest X over the rows of event e, arg int32 [B, D] the row it came from (the first
 *   row wins a tie); an event without rows: 0 and -1.  wfs_event_max_bwd: dX [n_cap, D] = dY where arg names the row, else 0. */
int wfs_graph_kmax(void);
int wfs_graph_knn_host(const int32_t *coords, int64_t n, int64_t n_valid, int32_t k, int32_t self_loop, int32_t *nbr,
                       int32_t *deg);
int wfs_graph_knn(const int32_t *coords, int64_t n_cap, const int64_t *n_dev, int32_t k, int32_t self_loop, int32_t *nbr,
                  int32_t *deg, int32_t *rev_pos, int32_t *rev_rows, void *stream);
int wfs_film_message_fwd(const void *P, const int32_t *nbr, const int32_t *deg, int64_t n_cap, int32_t D, void *out,
                         int32_t dtype, const int64_t *n_dev, void *stream);
int wfs_film_message_bwd(const void *P, const void *dout, const int32_t *nbr, const int32_t *deg, const int32_t *rev_pos,
                         const int32_t *rev_rows, int64_t n_cap, int32_t D, void *dP, int32_t dtype, const int64_t *n_dev,
                         void *stream);
int wfs_rows_zero_tail(void *X, int64_t n_cap, int32_t C, int32_t dtype, const int64_t *n_dev, void *stream);
int wfs_event_max_fwd(const int32_t *coords, const void *X, int64_t n_cap, int32_t D, int32_t B, void *Y, int32_t *arg,
                      int32_t dtype, const int64_t *n_dev, void *stream);
int wfs_event_max_bwd(const int32_t *coords, const void *dY, const int32_t *arg, int64_t n_cap, int32_t D, int32_t B,
                      void *dX, int32_t dtype, const int64_t *n_dev, void *stream);

/* ---- Classification metrics: accuracy, confusion matrix, cross-entropy mean, ROC tables (csrc/classmetrics.hip) ----
 * What the reference's LitPSD / LitSegClassifier keep per validation / test step: torchmetrics' Accuracy and
 * ConfusionMatrix(num_classes = n_type), and ROCCurve's binary confusion matrices of softmax(logits)[:, k] against T
 * thresholds (src/evaluation/ROCCurve.py) -- here for every class k at once.  Additions only: WFS_ABI_VERSION stays.
 *
 * wfs_class_metrics_accumulate: ONE launch on `stream`; no read-back, no allocation, no memset.
 *   logits      [N, C] of `dtype`, row r at logits + r * row_stride ELEMENTS (row_stride >= C); element alignment only
 *   labels      int64 [N]; a row whose label is ignore_index is counted in the head's "ignored" and nowhere else
 *   loss_mask   uint8 [N] or NULL: the cross-entropy term enters the loss sum only where it is non-zero
 *   N, n_dev    rows, and the optional device-side valid count (as everywhere): rows at and beyond it are not read
 *   thresholds  device float [T], ASCENDING; the callers fill it with (float)((i + 1.0) / T)
 *   tables      int64 [wfs_class_metrics_table_ints(C, T)], persistent, in this order:
 *                 head [5]            rows counted, rows correct, loss rows, loss sum, rows ignored
 *                 confusion [C, C]    [label, prediction]
 *                 roc [C, 2, T + 1]   [class k, label == k, b_k]
 *   flags       int32 [1], STICKY: 1 a non-finite logit in a counted row, 2 a label outside [0, C) that is not
 *               ignore_index, 4 a loss term of 2^15 or more, or the loss sum left int64.  A flagged row is in no table.
 *   max_blocks  0: the launch's own block count; the tables do not depend on it
 * Per counted row: prediction = the FIRST index of the largest logit; p_k = exp(x_k - m) / sum_j exp(x_j - m) in fp64 from
 * the stored logits, rounded once to float; b_k = #{i : p_k >= thresholds[i]} in 0 .. T; the loss term m + log(sum_j
 * exp(x_j - m)) - x_label in fp64, summed as round(term * WFS_SEG_FIXED_ONE).  Integer atomics only: the tables are
 * bit-identical from run to run and for every max_blocks.
 * Limits: 2 <= C <= 32, 1 <= T <= 1024 and 6 + C * C + 2 * C * (T + 1) + T <= 16384 (the workgroup's 64 KB LDS image);
 * outside them wfs_class_metrics_table_ints returns 0 and the accumulate WFS_EINVAL. */
#define WFS_CLASS_METRICS_MAX_CLASSES 32
#define WFS_CLASS_METRICS_MAX_THRESH 1024
#define WFS_CLASS_METRICS_LDS_BYTES 65536
size_t wfs_class_metrics_table_ints(int32_t C, int32_t T);
int wfs_class_metrics_accumulate(const void *logits, int32_t dtype, int64_t row_stride, const int64_t *labels,
                                 int64_t ignore_index, const uint8_t *loss_mask, int64_t N, const int64_t *n_dev,
                                 int32_t C, const float *thresholds, int32_t T, int64_t *tables, int32_t *flags,
                                 int32_t max_blocks, void *stream);

/* opt-in per-kernel timing (HIP events on the launch stream), used by bench.py's roofline ---- */
#define WFS_TIMER_GATHER_CONV 0
#define WFS_TIMER_GATHER_DW 1
#define WFS_TIMER_RULEBOOK 2
#define WFS_TIMER_CONV_BACKWARD 3   /* wfs_conv_backward's one-launch form (dW + dX) */
#define WFS_TIMER_COUNT 4
int wfs_timing_enable(int32_t on);                        /* also clears the table            */
int wfs_timing_read(int32_t timer, double *total_ms, int64_t *launches);  /* synchronises     */

#ifdef __cplusplus
}
#endif
#endif /* WFSPARSE_H */
