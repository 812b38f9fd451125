/* fourq_amd -- batched FourQ (Curve4Q) scalar multiplication on AMD MI355X (gfx950).
 *
 * C ABI of libfourq_amd.so.  This is the drop-in boundary for the hot path of the reference
 * implementation bifurcation/fourq (pure Python; citations are impl/<file>:<line>).  The
 * reference has no FFI of its own -- its boundary is the Python signatures
 *     MUL_windowed(m, P, table=None)   curve4q.py:188      table_windowed(P)   curve4q.py:179
 *     MUL_endo(m, P, table=None)       curve4q.py:405      table_endo(P)       curve4q.py:385
 *     DH_windowed / DH_endo            curve4q.py:464-468  (DH_core curve4q.py:446)
 * so each entry point below is the batched form of one of those, and the ctypes stub that
 * presents the reference signatures on top of it is fourq_amd/curve4q.py.
 *
 * Data layout (all little-endian 64-bit words; plain pointers, caller-allocated):
 *   GF(p) element      2 words, value in [0, 2^128) accepted, canonical [0, p) returned
 *   GF(p^2) element    4 words  (re, im)                         fields.py:134
 *   scalar             4 words  (256-bit, as the reference's KAT generator curve4q.py:552-559)
 *   affine point       8 words  (x, y)
 *   R1 point          20 words  (X, Y, Z, Ta, Tb)                curve4q.py:100-106
 *   R2 point          16 words  (X+Y, Y-X, 2Z, 2dT)              curve4q.py:109-116
 *   table            128 words  8 R2 points                      curve4q.py:179-185, :385-403
 *
 * Every function returns FOURQ_OK (0) or a negative error code and never throws.  A context is
 * bound to one device and one HIP stream; calls on one context must not overlap, different
 * contexts are independent.  There is no CPU fallback: without a usable gfx950 device
 * fourq_ctx_create fails.
 *
 * A context owns device scratch (per-lane look-up tables, staging) that its launches reuse in stream order:
 * let the current stream's work finish (fourq_ctx_sync or the caller's own synchronisation) before handing the
 * context another stream with fourq_ctx_set_stream (the staged fixed-base tables are re-staged on the new stream).
 *
 * Pointer flavours: functions ending in _dev take DEVICE pointers, enqueue on the context's
 * stream and return without synchronising (use fourq_ctx_sync or the caller's stream).  The same
 * names without _dev take HOST pointers and are synchronous (H2D copy, kernel, D2H copy, pipelined over chunks of
 * the batch on three streams; see fourq_host_alloc for the fast path).
 * Device arrays are read and written as 16-byte vectors: every array pointer handed to a _dev function must be
 * 16-byte aligned (FOURQ_ERR_INVALID otherwise; hipMalloc / fourq_dev_alloc / torch allocations are).  Host
 * pointers need no particular alignment.
 */
#ifndef FOURQ_AMD_H
#define FOURQ_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FOURQ_OK 0
#define FOURQ_ERR_INVALID (-1)   /* NULL pointer, bad size or bad enum */
#define FOURQ_ERR_NODEVICE (-2)  /* no HIP device / device is not gfx950-compatible */
#define FOURQ_ERR_NOMEM (-3)     /* device or host allocation failed */
#define FOURQ_ERR_HIP (-4)       /* a HIP runtime call or kernel launch failed (see fourq_last_error) */

/* per-element status of the DH entry points; the Python wrapper re-raises 1 and 2 with the
 * reference's exact messages (curve4q.py:448, :460) */
#define FOURQ_DH_OK 0
#define FOURQ_DH_NOT_ON_CURVE 1
#define FOURQ_DH_NEUTRAL 2

/* largest batch any entry point accepts (the kernels' 32-bit element counters round n up to whole 256-lane blocks) */
#define FOURQ_MAX_BATCH 0xffffff00u
#define FOURQ_BYTES_DECODE_BASE 16  /* status of the *_bytes_* calls: this + FOURQ_DECODE_* when an encoded point does not decode */

#define FOURQ_SCALAR_WORDS 4
#define FOURQ_AFFINE_WORDS 8
#define FOURQ_R1_WORDS 20
#define FOURQ_R2_WORDS 16
#define FOURQ_TABLE_WORDS 128

typedef struct fourq_ctx fourq_ctx;

/* ---- library / context ---------------------------------------------------------------------- */
/* The ABI this header describes.  Structs that the library fills (fourq_host_stats) and prototypes may grow between versions: a host
 * compiled against this header must check fourq_version() == FOURQ_ABI_VERSION once at start-up (the Python binding does, fourq_amd/_lib.py)
 * -- or use the size-carrying forms (fourq_ctx_host_stats_sized), which never write past what the caller's header knew. */
#define FOURQ_ABI_VERSION 600
int fourq_version(void);                       /* 10000*major + 100*minor + patch; == FOURQ_ABI_VERSION for a matching library */
const char *fourq_build_id(void);              /* 16 hex digits: hash of the sources and flags the library was built from */
const char *fourq_strerror(int code);
const char *fourq_last_error(const fourq_ctx *ctx);   /* detail of the last FOURQ_ERR_HIP */

/* Number of usable devices (gfx950 only; 0 when there is none -- not an error).  SURVEY.md 8(e): one context per device,
 * contiguous shards, no exchange step; fourq_amd/multi.py (MultiEngine) is the host-side loop over them. */
int fourq_device_count(int *count);
int fourq_ctx_create(int device, fourq_ctx **out);
/* Threads.  Every entry point that takes a context holds that context's lock for its duration, so calls made on ONE context
 * from several threads are safe and take turns (a host-array call for its whole duration, a _dev call for its enqueue); the
 * reference's functions are pure, and a drop-in caller may use them from any thread.  Calls on different contexts run side by
 * side (fourq_amd/multi.py: one context and one host thread per device).  What stays per context and is therefore "of the last
 * call, whoever made it": fourq_last_error, fourq_ctx_host_stats, the stream and mode switches.  fourq_ctx_destroy waits for a
 * call in flight; starting another one after it is the caller's error. */
int fourq_ctx_destroy(fourq_ctx *ctx);
/* Use the caller's hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL restores the
 * context's own stream.  The context never synchronises an external stream behind the caller's back. */
int fourq_ctx_set_stream(fourq_ctx *ctx, void *hip_stream);
int fourq_ctx_sync(fourq_ctx *ctx);
/* Constant-time table selection (draft-ladd-cfrg-4q.md:753-758: "memory addresses accessed [must] not depend on secret
 * data").  OFF by default: the ladders then do exactly what the reference does -- a digit of the scalar is a table
 * address (curve4q.py:232, :440) and the SIGN of the digit is applied by masked selects (curve4q.py:193-206), never by
 * an address -- which is NOT constant-time with respect to the scalar's digits.  ON (this call, or
 * FOURQ_CT_SELECT=1 in the environment when the context is created): every ladder step reads the whole table and
 * keeps the wanted entry by masks; per-lane tables live in registers; signs are applied arithmetically.  Results are
 * bit-identical in both modes; the price of ON is in DESIGN.md section 10.
 * Environment: FOURQ_CT_SELECT is the ONE variable the library reads as a product option.  The variables that steer batches onto
 * particular kernels (FOURQ_MIXED_ROUND, FOURQ_PAIR_MAX, FOURQ_QUAD_MAX, FOURQ_MIXED_QUEUE, FOURQ_NORM_K, FOURQ_BLOCKS_PER_CU,
 * FOURQ_HOST_BOUNCE, FOURQ_HOST_ZERO_COPY, FOURQ_PIPE_SLOTS, FOURQ_PIPE_GENS, FOURQ_PIPE_HOST_WAIT, FOURQ_PIPE_HOST_POLL, FOURQ_PIPE_MEASURE, FOURQ_FUSED_IO) are test hooks: they are ignored unless FOURQ_DEBUG_ROUTES=1 is set (tools/README.md).
 * One variable of the HIP RUNTIME matters to the host-pointer calls: they overlap copy-in, kernels and copy-out on three streams,
 * and the runtime shares GPU_MAX_HW_QUEUES hardware queues (default 4) among all streams the process uses -- in a process with two
 * or more other busy streams the three stages take turns and a large call takes up to twice as long.  Set GPU_MAX_HW_QUEUES=8 in
 * the host's environment before its first HIP call (the library does not touch the environment; the Python package sets it at
 * import when it is unset).  The _dev calls use one stream and are not affected.  INTEGRATION.md section 3. */
int fourq_ctx_set_ct_select(fourq_ctx *ctx, int on);
int fourq_ctx_get_ct_select(const fourq_ctx *ctx, int *on);
/* Resident lanes the ladder kernels are launched with (scratch is sized for this many). */
int fourq_ctx_lanes(const fourq_ctx *ctx, size_t *lanes);
/* Buffer growth.  The context owns the intermediates of the DH and protocol-level calls (deferred-normalisation planes,
 * decoded keys, first-half results); they grow on demand, and a _dev call whose batch is larger than any seen before
 * SYNCHRONISES the context's stream and reallocates before it enqueues (such a call cannot be captured into a HIP graph).
 * fourq_ctx_reserve(ctx, n) sizes them once for batches of up to n elements: afterwards _dev calls of at most n elements
 * only enqueue.  (The host-pointer calls size their pipeline slots themselves and are synchronous anyway.)
 * Capturing _dev calls into a HIP graph: reserve first, and STAGE the caller's tables first -- a fixed-base table or a comb is
 * uploaded from a context-owned host copy when it differs from what is staged, and that upload must not be captured (it would
 * read the mutable copy at replay time).  One un-captured call with the same table (or fourq_comb_stage) stages it; a call that
 * would have to stage while its stream is being captured returns FOURQ_ERR_HIP with fourq_last_error() saying so. */
int fourq_ctx_reserve(fourq_ctx *ctx, size_t n);

/* Pinned (page-locked) host memory.  The host-pointer batch calls cut their arrays into chunks and overlap the
 * H2D copy, the kernels and the D2H copy of consecutive chunks; arrays that live in pinned memory (from here, from
 * hipHostMalloc or from torch's pin_memory) are moved by DMA straight from / to the caller's buffer at the link's
 * rate, pageable arrays take an extra pass through pinned bounce buffers filled by host threads. */
int fourq_host_alloc(fourq_ctx *ctx, size_t bytes, void **out);
int fourq_host_free(fourq_ctx *ctx, void *ptr);
/* transfer statistics of the context's last host-pointer batch call */
typedef struct fourq_host_stats {
    double h2d_ms, d2h_ms;          /* summed durations of the chunk copies (HIP events), measured only while
                                     * fourq_ctx_set_host_timing(ctx, 1) is in force -- 0 otherwise: the six event records per
                                     * chunk are not free, so a production call does not make them (also 0 for a call of at
                                     * most 64 KiB: its kernels read and write a pinned host buffer in place, there are no
                                     * device copies at all) */
    uint64_t h2d_bytes, d2h_bytes;  /* bytes moved by device copies: 0 for such an in-place call */
    uint32_t chunks;
    int pinned_in, pinned_out;      /* 1: every input / output array was pinned (no bounce copy) */
    double kernels_ms;              /* under fourq_ctx_set_host_timing: summed over the chunks, from "the kernel stream has the chunk's
                                     * bytes" to "the chunk's kernels are done" (HIP events on the kernel stream); 0 otherwise */
    double kernels_span_ms;         /* ... and from the first chunk's start to the last chunk's end: span - sum = the kernel stream's idle
                                     * time between chunks (waiting for bytes, launch gaps) */
    /* 0.6.0: what the call's chunks were PLANNED with (fourq_amd/csrc/pipeline_plan.h) -- the context's own measurements of this route in this
     * selection mode when planned_from_measurement is 1 (every multi-chunk call times one middle chunk and leaves the figures for the next
     * call of the same route), the compiled-in first-call guesses when 0 -- and what THIS call measured.  0 for a call of one chunk. */
    double planned_kernel_ns_per_elem, planned_link_in_gbs, planned_link_out_gbs;   /* kernel time per element; link rate each way, GB/s = bytes / ns */
    double measured_kernel_ns_per_elem;
    int planned_from_measurement;
} fourq_host_stats;
int fourq_ctx_host_stats(const fourq_ctx *ctx, fourq_host_stats *out);
/* The same, writing at most `size` bytes (pass sizeof(fourq_host_stats) of the header the caller was compiled against): safe across
 * versions in which the struct grew (0.4.0: 48 bytes, 0.5.0: 64, 0.6.0: 104). */
int fourq_ctx_host_stats_sized(const fourq_ctx *ctx, void *out, size_t size);
/* Diagnostic: time the chunk copies of the following host-pointer calls (h2d_ms / d2h_ms above).  OFF by default; bytes, chunk
 * count and the pinned flags are always reported. */
int fourq_ctx_set_host_timing(fourq_ctx *ctx, int on);
/* Diagnostic: where chunk `chunk` of the context's last host-pointer call sat in time, when that call was made under
 * fourq_ctx_set_host_timing -- six stamps in milliseconds since the call's first event: copy-in start, copy-in end, copy-out start,
 * copy-out end, kernels start (the kernel stream is past its wait for the chunk's bytes), kernels end.  FOURQ_ERR_INVALID past the
 * last timed chunk (tools/pipeline_chunks.py prints the table). */
int fourq_ctx_host_chunk_stamps(const fourq_ctx *ctx, uint32_t chunk, double out_ms[6]);

/* Diagnostic: the shader clock (MHz) the device holds at this moment, measured from inside a kernel -- a 16-wave probe on a stream of
 * the context's own times `window_us` (1 .. 1 000 000) of the constant 100 MHz counter (s_memrealtime) in shader cycles (s_memtime);
 * median, minimum and maximum over the probe's waves (two per XCD).  Called while the context's stream has work queued for longer than
 * the window (the _dev calls only enqueue) it reports the clock under that load: a time measured on one box times this clock is a cycle
 * count comparable with another box's (devices differ by several percent in the clock they hold under the same kernel).  Synchronous
 * for the window; no product kernel carries a stamp.  mhz_min / mhz_max / under_load may be NULL.  *under_load = 1 when the context's
 * stream still had work in flight when the window closed, 0 when it had already drained (or the probe had queued BEHIND it on a shared
 * hardware queue): the reading is then the clock of an idle chip and must not be used to convert the load's time into cycles. */
int fourq_diag_clock(fourq_ctx *ctx, uint32_t window_us, double *mhz_median, double *mhz_min, double *mhz_max, int *under_load);
/* The clock OF a stretch of work, as a bracket: _begin and _stop each enqueue one tiny kernel on the CONTEXT'S stream -- before and behind
 * whatever the caller enqueues in between (_dev calls), so the host never waits and nothing stays resident beside the work -- whose waves
 * record their CU's cycle counter and the global 100 MHz counter; _end (implies _stop) waits for the stream, pairs the two launches' stamps
 * CU by CU (s_memtime is a per-CU counter) and returns the median clock over the CUs, its 5th / 95th percentile as min / max, and the
 * length of the window in microseconds.  bench.py brackets its timed steps with it; no product kernel carries a stamp. */
int fourq_diag_clock_begin(fourq_ctx *ctx);
int fourq_diag_clock_stop(fourq_ctx *ctx);
int fourq_diag_clock_end(fourq_ctx *ctx, double *mhz_median, double *mhz_min, double *mhz_max, double *window_us);

/* Plain device-memory helpers so that a host program without a HIP binding can use the _dev API. */
int fourq_dev_alloc(fourq_ctx *ctx, size_t bytes, void **out);
int fourq_dev_free(fourq_ctx *ctx, void *ptr);
int fourq_dev_upload(fourq_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
int fourq_dev_download(fourq_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);

/* ---- look-up tables: table_windowed(P) curve4q.py:179, table_endo(P) curve4q.py:385 -----------
 * Host pointers; synchronous: they run behind whatever the context's stream still holds and wait for it.  Building a table (these two and
 * fourq_comb_table) does not change what the context has STAGED: the fixed-base table of the last fixed-base call and the comb that
 * comb == NULL stands for are the same before and after. */
int fourq_table_windowed(fourq_ctx *ctx, const uint64_t *p_r1, uint64_t *table);
int fourq_table_endo(fourq_ctx *ctx, const uint64_t *p_r1, uint64_t *table);

/* ---- variable-base scalar multiplication: MUL_*(m_i, P_i), table=None ------------------------- */
/* out_r1[i] = raw R1 tuple the reference returns (curve4q.py:235, :442), n x 20 words */
int fourq_mul_endo_batch(fourq_ctx *ctx, const uint64_t *scalars, const uint64_t *points_r1, uint64_t *out_r1, size_t n);
int fourq_mul_windowed_batch(fourq_ctx *ctx, const uint64_t *scalars, const uint64_t *points_r1, uint64_t *out_r1, size_t n);
int fourq_mul_endo_batch_dev(fourq_ctx *ctx, const uint64_t *scalars, const uint64_t *points_r1, uint64_t *out_r1, size_t n);
int fourq_mul_windowed_batch_dev(fourq_ctx *ctx, const uint64_t *scalars, const uint64_t *points_r1, uint64_t *out_r1, size_t n);

/* ---- the same with affine / encoded I/O ("affine-only I/O variant") ----------------
 * out_affine[i] = R1toAffine(MUL_<algo>(m_i, AffineToR1(x_i, y_i)))   curve4q.py:100-106; canonical affine, n x 8 words: 160 bytes per
 * operation across the ABI instead of 352.  Like MUL_* itself these check nothing: a point outside the prime-order subgroup gives the
 * reference's (meaningless) answer (draft-ladd-cfrg-4q.md:467-468). */
int fourq_mul_endo_affine_batch(fourq_ctx *ctx, const uint64_t *scalars, const uint64_t *points_affine, uint64_t *out_affine, size_t n);
int fourq_mul_windowed_affine_batch(fourq_ctx *ctx, const uint64_t *scalars, const uint64_t *points_affine, uint64_t *out_affine, size_t n);
int fourq_mul_endo_affine_batch_dev(fourq_ctx *ctx, const uint64_t *scalars, const uint64_t *points_affine, uint64_t *out_affine, size_t n);
int fourq_mul_windowed_affine_batch_dev(fourq_ctx *ctx, const uint64_t *scalars, const uint64_t *points_affine, uint64_t *out_affine, size_t n);
/* out32[i] = encode(R1toAffine(MUL_<algo>(m_i, AffineToR1(decode(points32[i])))))   curve4q.py:41-96: 96 bytes per operation.
 * status[i]: 0 ok; FOURQ_BYTES_DECODE_BASE + FOURQ_DECODE_* when points32[i] does not decode (out32[i] is all zero then). */
int fourq_mul_endo_bytes_batch(fourq_ctx *ctx, const uint64_t *scalars, const uint8_t *points32, uint8_t *out32, uint8_t *status, size_t n);
int fourq_mul_windowed_bytes_batch(fourq_ctx *ctx, const uint64_t *scalars, const uint8_t *points32, uint8_t *out32, uint8_t *status, size_t n);
int fourq_mul_endo_bytes_batch_dev(fourq_ctx *ctx, const uint64_t *scalars, const uint8_t *points32, uint8_t *out32, uint8_t *status, size_t n);
int fourq_mul_windowed_bytes_batch_dev(fourq_ctx *ctx, const uint64_t *scalars, const uint8_t *points32, uint8_t *out32, uint8_t *status, size_t n);

/* ---- fixed-base scalar multiplication: MUL_*(m_i, P, table=T) --------------------------------- */
/* `table` is 128 words (host pointer in both flavours: it is 1 KiB and is staged once per call) */
int fourq_mul_endo_fixed_batch(fourq_ctx *ctx, const uint64_t *scalars, const uint64_t *table, uint64_t *out_r1, size_t n);
int fourq_mul_windowed_fixed_batch(fourq_ctx *ctx, const uint64_t *scalars, const uint64_t *table, uint64_t *out_r1, size_t n);
int fourq_mul_endo_fixed_batch_dev(fourq_ctx *ctx, const uint64_t *scalars, const uint64_t *table, uint64_t *out_r1, size_t n);
int fourq_mul_windowed_fixed_batch_dev(fourq_ctx *ctx, const uint64_t *scalars, const uint64_t *table, uint64_t *out_r1, size_t n);

/* ---- mixed batch (BASELINE.json config 5): element i is fixed-base (flags[i] == 0, uses `table`)
 *      or variable-base (flags[i] != 0, uses points_r1[i]); MUL_endo in both cases ---------------- */
int fourq_mul_endo_mixed_batch(fourq_ctx *ctx, const uint64_t *scalars, const uint64_t *points_r1, const uint8_t *flags,
                               const uint64_t *table, uint64_t *out_r1, size_t n);
int fourq_mul_endo_mixed_batch_dev(fourq_ctx *ctx, const uint64_t *scalars, const uint64_t *points_r1, const uint8_t *flags,
                                   const uint64_t *table, uint64_t *out_r1, size_t n);

/* ---- Diffie-Hellman: DH_core(m_i, P_i, mul, table) curve4q.py:446-462 --------------------------
 * table == NULL: variable base (the table is built from [392]P_i); otherwise `table` (host pointer)
 * is used for every element exactly as the reference does (it ignores the point, curve4q.py:209, :426).
 * status[i]: FOURQ_DH_*; out_affine[i] is all zero when status[i] != 0.
 * Large batches share one GFp.inv (fields.py:66-106) among up to eight elements of R1toAffine (curve4q.py:103-106;
 * Montgomery's trick); the affine result is canonical and therefore unchanged. */
int fourq_dh_endo_batch(fourq_ctx *ctx, const uint64_t *scalars, const uint64_t *points_affine, const uint64_t *table,
                        uint64_t *out_affine, uint8_t *status, size_t n);
int fourq_dh_windowed_batch(fourq_ctx *ctx, const uint64_t *scalars, const uint64_t *points_affine, const uint64_t *table,
                            uint64_t *out_affine, uint8_t *status, size_t n);
int fourq_dh_endo_batch_dev(fourq_ctx *ctx, const uint64_t *scalars, const uint64_t *points_affine, const uint64_t *table,
                            uint64_t *out_affine, uint8_t *status, size_t n);
int fourq_dh_windowed_batch_dev(fourq_ctx *ctx, const uint64_t *scalars, const uint64_t *points_affine, const uint64_t *table,
                                uint64_t *out_affine, uint8_t *status, size_t n);

/* ---- the protocol step on the device: 32-byte public keys in, 32-byte shared secrets out -----------------------
 * out32[i] = encode(DH_<algo>(m_i, decode(keys32[i]) [, table]))   draft-ladd-cfrg-4q.md:707-723;
 * curve4q.py:49-96 (decode), :446-462 (DH_core), :41-46 (encode).  Decoded points and shared points never leave the
 * GPU.  status[i]: 0 ok; FOURQ_DH_NOT_ON_CURVE / FOURQ_DH_NEUTRAL from the DH stage; 16 + FOURQ_DECODE_* when the
 * key does not decode (takes precedence).  out32[i] is all zero unless status[i] == 0. */
int fourq_dh_endo_bytes_batch(fourq_ctx *ctx, const uint64_t *scalars, const uint8_t *keys32, const uint64_t *table,
                              uint8_t *out32, uint8_t *status, size_t n);
int fourq_dh_windowed_bytes_batch(fourq_ctx *ctx, const uint64_t *scalars, const uint8_t *keys32, const uint64_t *table,
                                  uint8_t *out32, uint8_t *status, size_t n);
int fourq_dh_endo_bytes_batch_dev(fourq_ctx *ctx, const uint64_t *scalars, const uint8_t *keys32, const uint64_t *table,
                                  uint8_t *out32, uint8_t *status, size_t n);
int fourq_dh_windowed_bytes_batch_dev(fourq_ctx *ctx, const uint64_t *scalars, const uint8_t *keys32, const uint64_t *table,
                                      uint8_t *out32, uint8_t *status, size_t n);
/* One exchange per element: out[i] = DH_endo(a_i, DH_endo(b_i, base [, table392])) -- the pattern of curve4q.py:731
 * (BASELINE.json "dh_exchange"); `base_affine` (8 words) and `table392` = table_endo([392]base) or NULL are HOST
 * pointers in both flavours.  The first half's results stay on the device.  status[i]: first failure of either half. */
int fourq_dh_exchange_batch(fourq_ctx *ctx, const uint64_t *a_scalars, const uint64_t *b_scalars, const uint64_t *base_affine,
                            const uint64_t *table392, uint64_t *out_affine, uint8_t *status, size_t n);
int fourq_dh_exchange_batch_dev(fourq_ctx *ctx, const uint64_t *a_scalars, const uint64_t *b_scalars, const uint64_t *base_affine,
                                const uint64_t *table392, uint64_t *out_affine, uint8_t *status, size_t n);

/* ---- point compression: encode(X, Y) curve4q.py:41, decode(B) curve4q.py:49 -----------------------
 * 32 bytes per point: y0 | y1 little-endian, sign(x) in the top bit of the last byte.  decode reports, per
 * element, the exception the reference would raise; out_affine[i] is all zero unless status[i] == 0. */
#define FOURQ_DECODE_OK 0
#define FOURQ_DECODE_RESERVED_BIT 1        /* "Malformed point: reserved bit is not zero" (curve4q.py:53, :62) */
#define FOURQ_DECODE_NOT_ON_CURVE 2        /* "Point not on curve" (curve4q.py:94) */
#define FOURQ_DECODE_REF_ATTRIBUTE_ERROR 3 /* the reference's t == 0 branch (curve4q.py:76-77) raises AttributeError */
int fourq_encode_batch(fourq_ctx *ctx, const uint64_t *points_affine, uint8_t *out32, size_t n);
int fourq_decode_batch(fourq_ctx *ctx, const uint8_t *in32, uint64_t *out_affine, uint8_t *status, size_t n);
int fourq_encode_batch_dev(fourq_ctx *ctx, const uint64_t *points_affine, uint8_t *out32, size_t n);
int fourq_decode_batch_dev(fourq_ctx *ctx, const uint8_t *in32, uint64_t *out_affine, uint8_t *status, size_t n);

/* ---- fixed-base comb (draft-ladd-cfrg-4q.md:725-729: "MAY use any method ... provided that it agrees") ------
 * A comb table (mLSB-set recoding, w = 9, v = 4: 1 024 points, held in one CU's LDS) for a base point B of order N makes [m]B
 * cost 6 doublings + 27 mixed additions instead of 64 + 64; the table object also holds an 80-point comb (w = v = 5) that the
 * constant-time mode scans in 16-entry blocks.  Outputs are canonical AFFINE points, identical to
 * R1toAffine(MUL_endo(m, B)); the un-normalised R1 tuple of the reference is NOT reproduced, so this serves the
 * DH/keygen side (DH_endo(m, G, table) == fourq_comb_mul_batch with the comb of [392]G), not raw MUL_*.
 * comb table: FOURQ_COMB_WORDS words = 1 024 + 80 entries x (x+y, y-x, 2d*x*y), 4 words each (103.5 KiB). */
#define FOURQ_COMB_POINTS 1104
#define FOURQ_COMB_WORDS (1104 * 12)
/* Builds and returns the table; it is neither staged nor does it disturb the staged one (see "look-up tables" above). */
int fourq_comb_table(fourq_ctx *ctx, const uint64_t *p_r1, uint64_t *comb);
/* The device copy of the comb stays staged between calls.  A batch call with a non-NULL `comb` compares it with the staged
 * copy (103.5 KiB on the host, per call) and uploads it when it differs; fourq_comb_stage does that once, and batch calls
 * with comb == NULL then use the staged table without touching it (FOURQ_ERR_INVALID when no table was ever given; after
 * fourq_ctx_set_stream the context uploads its own copy again by itself on the first use). */
int fourq_comb_stage(fourq_ctx *ctx, const uint64_t *comb);
/* status[i]: FOURQ_DH_OK or FOURQ_DH_NEUTRAL ([m]B is the neutral point); out zeroed in that case */
int fourq_comb_mul_batch(fourq_ctx *ctx, const uint64_t *scalars, const uint64_t *comb, uint64_t *out_affine, uint8_t *status, size_t n);
int fourq_comb_mul_batch_dev(fourq_ctx *ctx, const uint64_t *scalars, const uint64_t *comb, uint64_t *out_affine, uint8_t *status, size_t n);
/* One exchange per element with the key-generation half through the comb: out[i] = DH_endo(a_i, K_i) with
 * K_i = [b_i]B affine = DH_endo(b_i, base, table_endo([392]base)) for the comb of B = [392]base (draft :725-729: any method
 * that agrees) -- BASELINE.json "dh_exchange" as bench.py's cfg4 runs it, as ONE call; the public keys K stay on the device.
 * `comb` as in fourq_comb_mul_batch (NULL = the staged table).  status[i]: first failure of either half. */
int fourq_dh_exchange_comb_batch(fourq_ctx *ctx, const uint64_t *a_scalars, const uint64_t *b_scalars, const uint64_t *comb,
                                 uint64_t *out_affine, uint8_t *status, size_t n);
int fourq_dh_exchange_comb_batch_dev(fourq_ctx *ctx, const uint64_t *a_scalars, const uint64_t *b_scalars, const uint64_t *comb,
                                     uint64_t *out_affine, uint8_t *status, size_t n);

/* ---- double-scalar multiplication [k]B + [l]P: the curve part of a Schnorr-type verification R' = [s]B + [h]A (SchnorrQ) ------
 * The fixed half goes through the comb, the variable half through MUL_endo, and one kernel adds the two projective results with the
 * complete twisted-Edwards addition and lowers the sum; neither half is normalised on its own and nothing but the result leaves the
 * device.  This is the scalar-level call for a caller with a hash of its own (h = H(R, A, msg) computed elsewhere); with SHA-512 the
 * fourq_sig_* calls below take the bytes and hash on the device.  Scalars: any value in [0, 2^256), as MUL_endo and the comb take them.
 * `comb` as in fourq_comb_mul_batch: the table of B from fourq_comb_table (B of order N), NULL = the staged comb.
 *
 * out_affine[i] = R1toAffine(ADD(MUL_endo(k_i, B), R1toR2(MUL_endo(l_i, AffineToR1(P_i)))))  canonical, n x 8 words.
 * Checks nothing, like MUL_*; the neutral point is a result like any other ((0, 1): no status, nothing zeroed -- unlike
 * fourq_comb_mul_batch).  For a P_i that is not on the curve the value is unspecified; the other elements are not affected. */
int fourq_double_mul_affine_batch(fourq_ctx *ctx, const uint64_t *k_scalars, const uint64_t *comb, const uint64_t *l_scalars,
                                  const uint64_t *points_affine, uint64_t *out_affine, size_t n);
int fourq_double_mul_affine_batch_dev(fourq_ctx *ctx, const uint64_t *k_scalars, const uint64_t *comb, const uint64_t *l_scalars,
                                      const uint64_t *points_affine, uint64_t *out_affine, size_t n);
/* The same on 32-byte encodings: decode(points32[i]) in, encode(...) out.
 * status[i]: 0 | FOURQ_BYTES_DECODE_BASE + FOURQ_DECODE_* (out32[i] is all zero then). */
int fourq_double_mul_bytes_batch(fourq_ctx *ctx, const uint64_t *k_scalars, const uint64_t *comb, const uint64_t *l_scalars,
                                 const uint8_t *points32, uint8_t *out32, uint8_t *status, size_t n);
int fourq_double_mul_bytes_batch_dev(fourq_ctx *ctx, const uint64_t *k_scalars, const uint64_t *comb, const uint64_t *l_scalars,
                                     const uint8_t *points32, uint8_t *out32, uint8_t *status, size_t n);
/* ok[i] = 1 iff points32[i] decodes and encode([k_i]B + [l_i]decode(points32[i])) == expect32[i] byte for byte; else 0.
 * status[i] as above (why a 0 is a 0: a key that does not decode, or a plain mismatch).  expect32 is compared as bytes: a
 * non-canonical or reserved-bit encoding of the right point is a mismatch.  One byte + one status byte per element leave the device. */
int fourq_verify_bytes_batch(fourq_ctx *ctx, const uint64_t *k_scalars, const uint64_t *comb, const uint64_t *l_scalars,
                             const uint8_t *points32, const uint8_t *expect32, uint8_t *ok, uint8_t *status, size_t n);
int fourq_verify_bytes_batch_dev(fourq_ctx *ctx, const uint64_t *k_scalars, const uint64_t *comb, const uint64_t *l_scalars,
                                 const uint8_t *points32, const uint8_t *expect32, uint8_t *ok, uint8_t *status, size_t n);

/* ---- grouped multi-scalar multiplication: out[g] = sum_j [k_gj]P_gj, the only call that adds across elements ----------------------------
 * groups x group_size = n elements laid out group after group (element i belongs to group i / group_size); every group has the same
 * length.  A caller with ragged groups pads with scalar 0 (or calls fourq_raggedsum_* below, which takes the groups as they are and pays
 * for no pad): the addition is complete, so the neutral [0]P is an ordinary operand.  The pad
 * point is the neutral (0, 1) or any other point on the affine flavour, and any string that DECODES on the bytes flavour (a valid key;
 * the neutral's own encoding 01 00 .. 00 is refused by decode, FOURQ_DECODE_REF_ATTRIBUTE_ERROR, and would mark its group).
 *
 * out_affine[g] = R1toAffine(sum over j < group_size of MUL_endo(k_gj, AffineToR1(P_gj)))  canonical, groups x 8 words, the sum taken with
 * the complete twisted-Edwards addition; every order of folding gives the same canonical point.  Scalars: any value in [0, 2^256).
 * Checks nothing, like MUL_* and fourq_double_mul_*; the neutral point is a result like any other ((0, 1): no status, nothing zeroed).
 * On the device: MUL_endo over all n elements, fold passes that each turn m projective rows per group into ceil(m / 64), and one
 * R1toAffine per group; nothing but the `groups` results leaves the device.
 *
 * groups == 0: FOURQ_OK, nothing touched.  group_size == 0 with groups > 0, or groups * group_size (overflow-checked) above
 * FOURQ_MAX_BATCH: FOURQ_ERR_INVALID.  _dev: enqueues on the context's stream and returns; every array pointer 16-byte aligned
 * (status need not be); after fourq_ctx_reserve(ctx, n) a call of at most n elements allocates and synchronises nothing.  The host-array
 * calls are synchronous -- copy in, the _dev call, copy out -- WITHOUT the chunk overlap of the per-element calls: the pipeline's arrays
 * are per element and this output is per group. */
int fourq_msm_affine_batch(fourq_ctx *ctx, const uint64_t *scalars, const uint64_t *points_affine, uint64_t *out_affine, size_t groups,
                           size_t group_size);
int fourq_msm_affine_batch_dev(fourq_ctx *ctx, const uint64_t *scalars, const uint64_t *points_affine, uint64_t *out_affine, size_t groups,
                               size_t group_size);
/* The same on 32-byte encodings: decode(points32[i]) in, encode(...) out, groups x 32 bytes.
 * status[g]: 0 | FOURQ_BYTES_DECODE_BASE + the LARGEST FOURQ_DECODE_* among the group's elements (out32[g] is all zero then; the other
 * groups are not affected).  A maximum folds in any order; fourq_decode_batch over the group's encodings tells which element it was. */
int fourq_msm_bytes_batch(fourq_ctx *ctx, const uint64_t *scalars, const uint8_t *points32, uint8_t *out32, uint8_t *status, size_t groups,
                          size_t group_size);
int fourq_msm_bytes_batch_dev(fourq_ctx *ctx, const uint64_t *scalars, const uint8_t *points32, uint8_t *out32, uint8_t *status,
                              size_t groups, size_t group_size);

/* ---- ragged grouped sums: out[g] = sum over group g of [k_i]P_i, groups of ANY length, by a shape the context holds ---------------------
 * The sums of fourq_msm_* over groups whose lengths differ, 0 included, without padding: a padded row is a whole MUL_endo ladder, the pad
 * of the bytes flavour has to be a string that decodes, and an empty group cannot be padded into existence at all.  (The names say
 * raggedsum, not msm_ragged, for the reason the bucket route's say bucketsum: fourq_msm_* is, by name, the equal-length family of four.)
 *
 * The shape: groups + 1 ascending uint32 row offsets on the HOST with offsets[0] == 0; group g owns rows offsets[g] .. offsets[g + 1] - 1
 * of the n = offsets[groups] rows, and a length of 0 is legal anywhere -- first, last, several in a row, all of them.  The offsets are
 * public metadata.  fourq_raggedsum_shape_set validates them, plans every fold pass on the host -- level p holds max(1, ceil(L / 64)) rows
 * for a group of L rows in level p - 1, passes repeat until every group has one row, and each output row of a pass gets one descriptor
 * { first input row, count <= 64 } -- and uploads the descriptors (8 bytes per output row, beside 96-byte rows).  No kernel reads an offset or
 * derives an address from anything but a descriptor, so the geometry of every launch is known on the host, as for fourq_msm_*.
 * Synchronous; replaces the old shape only once the new one is complete.  FOURQ_ERR_INVALID, and the old shape stays: a NULL context
 * (refused before anything else is looked at) or NULL offsets; groups == 0; groups or n above FOURQ_MAX_BATCH; offsets[0] != 0; a descending
 * pair; a level of 2^32 rows or more (billions of groups shorter than two rows).  The shape is the context's own, like the key set: the
 * commitment bases, the key set, the staged comb and the staged tables are untouched, it survives fourq_ctx_set_stream and is freed with the
 * context.  fourq_raggedsum_shape_count: the installed shape's groups and rows, 0 and 0 when none was ever set.
 *
 * The calls take n and groups from the installed shape; with no shape they are FOURQ_ERR_INVALID.
 * out_affine[g] = R1toAffine(sum over the rows i of group g of MUL_endo(k_i, AffineToR1(P_i)))  canonical, groups x 8 words; scalars: any
 * value in [0, 2^256); checks nothing, like fourq_msm_affine_batch.  out32[g]: the encoding of that point; status[g]: 0 |
 * FOURQ_BYTES_DECODE_BASE + the LARGEST FOURQ_DECODE_* among the group's rows (out32[g] is all zero then; the other groups are not affected).
 * An EMPTY group yields the neutral as an ordinary result: (0, 1), or 01 00 .. 00 with status 0.  For every group the row is, byte for
 * byte, what fourq_msm_* returns on that group alone with group_size = its length, and on a shape of equal lengths the result is what
 * fourq_msm_* returns on the whole arrays.  A shape of nothing but empty groups is legal and launches no ladder.
 *
 * _dev: enqueues on the context's stream and returns; every array pointer 16-byte aligned (status need not be).  The work buffer of these
 * calls holds up to groups + n / 64 partial rows after the first pass -- more than fourq_msm_* keeps where groups are short or empty -- so
 * fourq_ctx_reserve does not cover it; fourq_raggedsum_shape_reserve(ctx) sizes it for the installed shape, and after it a _dev call
 * allocates and synchronises nothing and can be captured into a graph.  The host-array calls copy in, run and copy out in one piece,
 * as fourq_msm_* do.
 *
 * Cost, measured against fourq_msm_affine_batch_dev (profiles/msm_ragged_timing.txt, time as a fraction of msm_dev's, and msm_dev's own
 * run-to-run spread).  Against the same groups padded to the longest with scalar 0: 1 024 groups of 1 .. 127 rows (67 207 rows against
 * 130 048 padded) 0.80, spread 8.5 % -- both sides need two generations of 65 536 lanes, so the ladder saves less than the row count says;
 * 1 023 groups of 8 rows and one of 8 192: 0.25 ms against 36.6 ms, 0.007; 65 536 groups of 0 .. 2 rows: 0.54, spread 0.5 %.  Against
 * fourq_msm_* itself at equal lengths, which is what the descriptors cost: 1024 x 64 1.000, 256 x 256 1.001, 1 x 65536 0.998, each inside
 * msm_dev's spread (0.4, 0.1, 0.6 %).  fourq_raggedsum_shape_set takes 0.02 ms on the host for 1 024 groups and 0.19 ms for 65 536. */
int fourq_raggedsum_shape_set(fourq_ctx *ctx, const uint32_t *offsets, size_t groups);
int fourq_raggedsum_shape_count(const fourq_ctx *ctx, size_t *groups, size_t *rows);
int fourq_raggedsum_shape_reserve(fourq_ctx *ctx);
int fourq_raggedsum_affine(fourq_ctx *ctx, const uint64_t *scalars, const uint64_t *points_affine, uint64_t *out_affine);
int fourq_raggedsum_affine_dev(fourq_ctx *ctx, const uint64_t *scalars, const uint64_t *points_affine, uint64_t *out_affine);
int fourq_raggedsum_bytes(fourq_ctx *ctx, const uint64_t *scalars, const uint8_t *points32, uint8_t *out32, uint8_t *status);
int fourq_raggedsum_bytes_dev(fourq_ctx *ctx, const uint64_t *scalars, const uint8_t *points32, uint8_t *out32, uint8_t *status);

/* ---- sums across elements: the bucket route ---------------------------------------------------------------------------------------------
 * The same arrays and, byte for byte, the same outputs and status as fourq_msm_affine_batch / fourq_msm_bytes_batch above -- the neutral
 * as an ordinary result, FOURQ_BYTES_DECODE_BASE + the largest FOURQ_DECODE_* per group, a zero row for such a group, its neighbours
 * untouched -- by the bucket method (Pippenger) instead of one ladder per element: for large groups.  Scalars: any value in [0, 2^256).
 *
 * The identity behind it: decompose(k) gives v_0..v_3 < 2^64 with MUL_endo(k, P) = [v_0]P + [v_1]phi(P) + [v_2]psi(P) + [v_3]psi(phi(P)),
 * and phi, psi are homomorphisms, so  sum_i MUL_endo(k_i, P_i) = S_0 + phi(S_1) + psi(S_2) + psi(phi(S_3))  with  S_j = sum_i [v_j(k_i)]P_i:
 * four 64-bit bucket sums over the same points and three endomorphisms per GROUP.  It holds for every point the ladder route accepts, points
 * outside the order-N subgroup included (where MUL_endo(k, P) is not [k]P), which is why the bytes are the ladder route's.
 *
 * window: 0 = the library picks, by group_size, from a table measured on the device (profiles/bucket_sum_timing.txt), and runs the ladder
 * route (fourq_msm_*_dev) where no window beat it; 4..12 = the bucket route with windows of that many bits, at any group size; anything
 * else FOURQ_ERR_INVALID.  fourq_bucketsum_window(group_size) is what 0 stands for: 0 (the ladder route) or 4..12.
 * With constant-time selection on (fourq_ctx_set_ct_select) every call runs the ladder route whatever the window is: a bucket's address
 * is a digit of a scalar, and the scalars of a commitment are secrets; the bytes are the same either way.  (In the default mode the
 * ladders use digits as addresses too, so the bucket route gives up nothing more.)
 *
 * Argument rules as fourq_msm_*: groups == 0 is FOURQ_OK and touches nothing; group_size == 0 with groups > 0, or groups * group_size above
 * FOURQ_MAX_BATCH, FOURQ_ERR_INVALID; _dev: every array pointer 16-byte aligned (status need not be).  The intermediates -- per group
 * 4 * ceil(64 / window) columns of 2^window - 1 buckets, and one index per element and column -- live in the context's work buffer BEHIND
 * what fourq_msm_* keeps there; fourq_ctx_reserve does not cover them.  fourq_bucketsum_reserve(ctx, groups, group_size, window) does:
 * after it a _dev call of that shape and window (or, with the same window, of no more groups and no larger groups) allocates and
 * synchronises nothing, and the geometry of every launch, pass counts included, follows from (groups, group_size, window) on the host.
 * The host-array calls copy in, run and copy out in one piece, as fourq_msm_* do. */
int fourq_bucketsum_window(size_t group_size);
int fourq_bucketsum_reserve(fourq_ctx *ctx, size_t groups, size_t group_size, unsigned window);
int fourq_bucketsum_affine(fourq_ctx *ctx, const uint64_t *scalars, const uint64_t *points_affine, uint64_t *out_affine, size_t groups,
                           size_t group_size, unsigned window);
int fourq_bucketsum_affine_dev(fourq_ctx *ctx, const uint64_t *scalars, const uint64_t *points_affine, uint64_t *out_affine, size_t groups,
                               size_t group_size, unsigned window);
int fourq_bucketsum_bytes(fourq_ctx *ctx, const uint64_t *scalars, const uint8_t *points32, uint8_t *out32, uint8_t *status, size_t groups,
                          size_t group_size, unsigned window);
int fourq_bucketsum_bytes_dev(fourq_ctx *ctx, const uint64_t *scalars, const uint8_t *points32, uint8_t *out32, uint8_t *status,
                              size_t groups, size_t group_size, unsigned window);

/* ---- commitments over a fixed generator set: out[g] = sum_j [k_gj]B_j through one comb per generator -----------------------------------
 * Pedersen and vector commitments use the same generators B_0 .. B_{m-1} in every group.  The context holds one comb per generator (the
 * object of fourq_comb_table: 1 024 points + the 80 of the constant-time shape, as working limbs), and row j of every group goes through
 * comb j: 6 doublings and 27 mixed additions instead of a variable-base ladder, no points over the link, and constant-time selection
 * (fourq_ctx_set_ct_select) stays on this route -- the scalars of a commitment are secrets.
 *
 * fourq_commit_bases_set(ctx, points_affine, m): m x 8 canonical affine words on the HOST.  Builds the m combs on the device into one array
 * the context owns (m x FOURQ_COMB_POINTS x 144 bytes: 155 KiB per generator) and replaces any earlier set.  Synchronous.  The staged single
 * comb (fourq_comb_stage) and the staged tables are untouched.  m == 0 or m > FOURQ_COMMIT_MAX_BASES: FOURQ_ERR_INVALID, and the old set
 * stays.  The set survives fourq_ctx_set_stream (it is plain device memory, complete when the call returns) and is freed with the context.
 * Every base must have order N: like fourq_comb_table the call does not check it, and the result for any other base is unspecified
 * (for an even k the comb computes -[N - k]B, which is [k]B only where [N]B is the neutral).  The outputs of
 * fourq_hash_to_curve_* and every [t]G qualify.  fourq_commit_bases_count: the size of the set, 0 when none was ever set.
 *
 * scalars: groups x group_size rows of 4 words, group after group, as fourq_msm_* takes them; any value in [0, 2^256).  Row j of every group
 * multiplies base j; 1 <= group_size <= the set's size, and a shorter vector uses the first bases.
 * out_affine[g], for bases of order N, equals bit for bit what fourq_msm_affine_batch returns for the same scalars with the bases tiled
 * `groups` times; out32[g] is its encoding.  The neutral point is an ordinary result: (0, 1), or 01 00 .. 00.  There is no status array:
 * nothing is decoded.
 *
 * route: 0 = the library picks, by `groups`, from a table measured on the device (profiles/commit_timing.txt; fourq_commit_route(groups) is
 * what 0 stands for); 1 = staged: one block per CU with comb j in the CU's LDS, staged again only when a block's base changes -- for many
 * groups per base; 2 = gather: one lane per row, every entry read where it lies in the set's array -- for few groups per base (one group
 * of 4 096 bases is 4 096 combs with one row each); anything else FOURQ_ERR_INVALID.  With constant-time selection on, the route makes no
 * difference: a block stages its base's 80-point shape (11.5 KB) and every addition reads all 16 entries of its block of the table.  The
 * bytes are the same on every route and in both modes.
 *
 * Cost, measured against fourq_msm_affine_batch_dev over the tiled bases (profiles/commit_timing.txt, groups x group_size, time as a
 * fraction of msm_dev's, staged / gather): 32768 x 2: 0.351 / 0.348; 1024 x 64: 0.414 / 0.424; 65536 x 1: 0.342 / 0.335; 64 x 1024: 1.385 /
 * 0.489 -- the staged route is SLOWER than msm_dev there, four combs staged per block for 64 rows each; 1 x 4096: 35.4 / 0.798.  With
 * constant-time selection, 1024 x 64: 0.62 of msm_dev in that mode.  The operation count alone would give 0.22; the fold passes and the
 * lowering are the same on both sides.  The staged route beat the gather route by more than the spread of msm_dev's own timings at one measured
 * shape only, 1024 x 64 (2.3 % against 2.0 %); at 32768 and 65536 groups the two are within the spread.  So route 0 is the staged route from
 * 1 024 groups and the gather route below.  fourq_commit_bases_set took 0.33 ms per base: 21 ms for 64 bases, 339 ms for 1 024.
 *
 * A NULL context is refused before anything else is looked at.  groups == 0: FOURQ_OK, nothing touched.  FOURQ_ERR_INVALID: group_size == 0,
 * group_size above the set's size, no set, groups * group_size (overflow-checked) above FOURQ_MAX_BATCH, a route outside 0..2.  _dev: enqueues
 * on the context's stream and returns; both array pointers 16-byte aligned.  The intermediates (12 words per row and the fold's partial
 * sums) live in the context's work buffer; fourq_ctx_reserve does not cover them, fourq_commit_reserve(ctx, groups, group_size) does: after
 * it a _dev call of at most that shape allocates and synchronises nothing, and the geometry of every launch follows from (groups,
 * group_size, route) on the host.  The host-array calls copy in, run and copy out in one piece, as fourq_msm_* do. */
#define FOURQ_COMMIT_MAX_BASES 4096
int fourq_commit_bases_set(fourq_ctx *ctx, const uint64_t *points_affine, size_t m);
int fourq_commit_bases_count(const fourq_ctx *ctx, size_t *m);
int fourq_commit_route(size_t groups);
int fourq_commit_reserve(fourq_ctx *ctx, size_t groups, size_t group_size);
int fourq_commit_affine(fourq_ctx *ctx, const uint64_t *scalars, uint64_t *out_affine, size_t groups, size_t group_size, int route);
int fourq_commit_affine_dev(fourq_ctx *ctx, const uint64_t *scalars, uint64_t *out_affine, size_t groups, size_t group_size, int route);
int fourq_commit_bytes(fourq_ctx *ctx, const uint64_t *scalars, uint8_t *out32, size_t groups, size_t group_size, int route);
int fourq_commit_bytes_dev(fourq_ctx *ctx, const uint64_t *scalars, uint8_t *out32, size_t groups, size_t group_size, int route);

/* ---- signatures from bytes: SchnorrQ-shaped sign / verify with SHA-512 and the arithmetic modulo N on the device ---------------------
 * Nothing but byte arrays crosses the ABI -- secret keys, public keys, messages, signatures, one ok and one status byte per row -- and no
 * intermediate (the hash of the secret key, the nonce, the challenge, R as a point) is ever on the host.  With H = SHA-512, LE(x) the
 * little-endian integer of a byte string, G the generator (`comb` = fourq_comb_table of AffineToR1(Gx, Gy), or NULL = the staged comb):
 *   keygen(sk)           k = H(sk);  pk = encode([LE(k[0:32])]G)           (the 256-bit value is used unreduced, as MUL_endo takes it)
 *   sign(sk, pk, msg)    k = H(sk);  r = LE(H(k[32:64] || msg)) mod N;  R = encode([r]G);  h = LE(H(R || pk || msg)) mod N;
 *                        s = (r - LE(k[0:32]) h) mod N;  sig = R || s (s: 32 bytes little-endian).  pk is an input: it is neither
 *                        derived again nor checked against sk.
 *   verify(pk, msg, sig) ok = 0 with status FOURQ_SIG_S_RANGE when LE(sig[32:64]) >= N; ok = 0 with FOURQ_BYTES_DECODE_BASE + FOURQ_DECODE_*
 *                        when pk does not decode (takes precedence); otherwise ok = (encode([s]G + [h]decode(pk)) == sig[0:32]) byte for
 *                        byte -- fourq_verify_bytes_batch with k = s, l = h -- so a non-canonical R is a plain mismatch (ok 0, status 0).
 * This is the structure of SchnorrQ (Costello, Longa: "SchnorrQ: Schnorr signatures on FourQ"); byte-for-byte interoperability with
 * FourQlib's schnorrq.c is NOT claimed (no vectors of it were available to check against), and s < N is deliberately stricter than a
 * bit-length check: it is what rules out a second encoding (s + N still fits 32 bytes) of the same signature.
 * Messages: n rows of `stride` bytes (stride >= the longest row; 0 only when every length is 0, msgs may then be NULL); lens: n x uint32,
 * or NULL = every row is msg_len bytes.  A row is never read at or past its length.  The host-pointer calls return FOURQ_ERR_INVALID for a
 * length above `stride` or above FOURQ_SIG_MAX_MSG.  The _dev calls cannot look: they CLAMP a row's length to `stride`;
 * fourq_sig_verify_batch_dev reports such a row as ok = 0, status FOURQ_SIG_MSG_CLAMPED (unless the key does not decode), while
 * fourq_sha512_batch_dev and fourq_sig_sign_batch_dev, which have no status, hash the clamped row.  _dev base pointers are 16-byte
 * aligned (msgs and lens included), `stride` is arbitrary: rows that start 8- or 16-byte aligned are read by vector loads, others by bytes.
 * The secret scalar and the nonce meet no branch and no address that depends on their value, in both table-selection modes of the comb
 * only when fourq_ctx_set_ct_select is on (the comb's digits are addresses otherwise, as everywhere in this library). */
#define FOURQ_SIG_S_RANGE 32          /* status: LE(sig[32:64]) >= N */
#define FOURQ_SIG_MSG_CLAMPED 64      /* status of the _dev verify: the row's length exceeded `stride` and was clamped */
#define FOURQ_SIG_MAX_MSG (1u << 20)  /* per-row message bytes the host-pointer calls accept */
/* out64[i] = SHA-512(msgs[i][0 : len_i]) */
int fourq_sha512_batch(fourq_ctx *ctx, const uint8_t *msgs, size_t stride, const uint32_t *lens, size_t msg_len, uint8_t *out64, size_t n);
int fourq_sha512_batch_dev(fourq_ctx *ctx, const uint8_t *msgs, size_t stride, const uint32_t *lens, size_t msg_len, uint8_t *out64, size_t n);
int fourq_sig_keygen_batch(fourq_ctx *ctx, const uint8_t *sk32, const uint64_t *comb, uint8_t *pk32, size_t n);
int fourq_sig_keygen_batch_dev(fourq_ctx *ctx, const uint8_t *sk32, const uint64_t *comb, uint8_t *pk32, size_t n);
int fourq_sig_sign_batch(fourq_ctx *ctx, const uint8_t *sk32, const uint8_t *pk32, const uint64_t *comb,
                         const uint8_t *msgs, size_t stride, const uint32_t *lens, size_t msg_len, uint8_t *sig64, size_t n);
int fourq_sig_sign_batch_dev(fourq_ctx *ctx, const uint8_t *sk32, const uint8_t *pk32, const uint64_t *comb,
                             const uint8_t *msgs, size_t stride, const uint32_t *lens, size_t msg_len, uint8_t *sig64, size_t n);
int fourq_sig_verify_batch(fourq_ctx *ctx, const uint8_t *pk32, const uint64_t *comb,
                           const uint8_t *msgs, size_t stride, const uint32_t *lens, size_t msg_len,
                           const uint8_t *sig64, uint8_t *ok, uint8_t *status, size_t n);
int fourq_sig_verify_batch_dev(fourq_ctx *ctx, const uint8_t *pk32, const uint64_t *comb,
                               const uint8_t *msgs, size_t stride, const uint32_t *lens, size_t msg_len,
                               const uint8_t *sig64, uint8_t *ok, uint8_t *status, size_t n);

/* ---- signatures of registered keys: [s]G + [h]A_id through one comb per key ------------------------------------------------------------
 * A verifier of a validator set, a fleet's certificates or a CA list sees the same public keys again and again: A is as fixed as G.  The
 * context holds one comb per registered key (the object of fourq_commit_bases_set: FOURQ_COMB_POINTS x 144 bytes, 155 KiB per key, 620 MiB
 * for 4 096), rows name their key by index, and one kernel walks G's comb and key id's comb in ONE accumulator: 6 doublings + 54 mixed
 * additions instead of a comb, a variable-base MUL_endo ladder with its endomorphism table, and the combiner.
 *
 * fourq_keyset_set(ctx, pk32, m, key_status): m x 32 bytes on the HOST; key_status: m bytes on the host, or NULL.  Synchronous.  Decodes
 * the keys on the device, checks every decoded point for order N, builds one comb per accepted key and keeps the 32 bytes and the status
 * byte of every slot on the device.  The old set is replaced only once the new one is complete.  The set is its own: the commitment bases,
 * the staged comb and the staged tables are untouched; it survives fourq_ctx_set_stream and is freed with the context.  m == 0 or
 * m > FOURQ_KEYSET_MAX_KEYS: FOURQ_ERR_INVALID, and the old set stays.  fourq_keyset_count: the size of the set, 0 when none was set.
 *   key_status[j]   0 accepted | FOURQ_BYTES_DECODE_BASE + FOURQ_DECODE_* when the bytes do not decode | FOURQ_KEYSET_NOT_ORDER_N when they
 *                   decode to a point A with [N]A != (0, 1).  A refused slot is still a slot of the set (the indices of the others do not
 *                   move); its comb is all zero and never contributes to a result.
 * Why the order check: for an even scalar the comb computes -[N - k]A, which is [k]A only for A of order N.  fourq_commit_bases_set leaves
 * that to its caller; public keys come from outside.  The check is [N]A by plain double-and-add with the complete addition (neither
 * MUL_endo nor MUL_windowed is [k]P outside the subgroup): (-x, -y) of an honest key, of order 2N, decodes and is refused here.  The
 * neutral point can never be a registered key: its encoding 01 00 .. 00, like those of the point of order 2 and of both points of order 4
 * (x0 = 0), does not decode (FOURQ_DECODE_REF_ATTRIBUTE_ERROR), so [N]O = O never reaches the order check.
 *
 * fourq_keyset_double_mul_bytes[_dev]: out32[i] = encode([k_i]B + [l_i]A_{id_i}); scalars any value in [0, 2^256); the neutral point is an
 * ordinary result (01 00 .. 00).  For an accepted key, out32 and status equal fourq_double_mul_bytes_batch on points32[i] = key[id_i] byte
 * for byte.
 * fourq_keyset_sig_verify[_dev]: h = LE(SHA-512(R || key_bytes[id] || msg)) mod N with the key bytes exactly as registered;
 * ok = (encode([s]G + [h]A_id) == R).  For an accepted key, ok and status equal fourq_sig_verify_batch on pk32[i] = key[id_i].  Messages
 * and their rules are those of fourq_sig_verify_batch[_dev].
 *   status[i], in this order of precedence:
 *     FOURQ_KEYSET_ID_RANGE    key_ids[i] >= the set's size.  The host-pointer calls can look and return FOURQ_ERR_INVALID instead; the _dev
 *                              calls clamp the index before it becomes an address, so nothing outside the set is read.
 *     the key's own status     FOURQ_BYTES_DECODE_BASE + FOURQ_DECODE_*, or FOURQ_KEYSET_NOT_ORDER_N
 *     FOURQ_SIG_MSG_CLAMPED    (_dev verify)
 *     FOURQ_SIG_S_RANGE        (verify)
 *   ok[i] = 0 for every non-zero status; out32[i] is all zero for the first two.
 * `comb`: the generator's table, or NULL = the staged comb, as everywhere.  A NULL context is refused before anything else is looked at.
 * n == 0: FOURQ_OK, nothing touched.  FOURQ_ERR_INVALID: no set installed, n > FOURQ_MAX_BATCH, a NULL array.  _dev: every array pointer
 * 16-byte aligned, key_ids included (status and ok need not be).  The intermediates live in the context's work buffer; fourq_ctx_reserve
 * does not cover them, fourq_keyset_reserve(ctx, n) does: after it a _dev call of at most n rows allocates and synchronises nothing, every
 * launch's geometry follows from n on the host, and the call can be captured into a graph.  The host-pointer calls run the chunked
 * pipeline, key_ids a 4-byte-per-row input.
 * Constant-time selection (fourq_ctx_set_ct_select): a verifier's inputs are public, but the scalar-level call may carry secrets, and a
 * gathered address is a digit.  With it on, both calls gather the rows' key BYTES by index and run the existing routes
 * (fourq_double_mul_bytes_batch_dev, fourq_sig_verify_batch_dev); statuses, bytes and ok are identical in both modes.
 * Cost, measured against fourq_sig_verify_batch_dev on the same rows, pk32 = keys[ids] (profiles/keyset_timing.txt; device-resident, 32-byte
 * messages, default mode; time as a fraction of the unkeyed call's, ids uniform random / sorted): 65536 rows: 0.419 / 0.421 over 1 key,
 * 0.429 / 0.426 over 16, 0.456 / 0.447 over 256, 0.470 / 0.482 over 4 096; 2^20 rows: 0.363 / 0.364, 0.363 / 0.363, 0.364 / 0.362 and
 * 0.372 / 0.362.  The spread of the unkeyed call's own timings was 0.0 to 4.0 %: the keyed route is faster by more than that at every
 * measured shape, none excepted -- the random gather over the 620 MiB of 4 096 combs costs 5 % at 65536 rows and 3 % at 2^20.  With
 * constant-time selection the time is the unkeyed route's plus the gather.  fourq_keyset_set took 0.33 ms per key: 22 ms for 64 keys,
 * 1.36 s for 4 096. */
#define FOURQ_KEYSET_MAX_KEYS 4096
#define FOURQ_KEYSET_NOT_ORDER_N 96   /* key / row status: the key decodes to a point whose order is not N */
#define FOURQ_KEYSET_ID_RANGE 112     /* row status of the _dev calls: key_ids[i] is not below the set's size */
int fourq_keyset_set(fourq_ctx *ctx, const uint8_t *pk32, size_t m, uint8_t *key_status);
int fourq_keyset_count(const fourq_ctx *ctx, size_t *m);
int fourq_keyset_reserve(fourq_ctx *ctx, size_t n);
int fourq_keyset_double_mul_bytes(fourq_ctx *ctx, const uint64_t *k_scalars, const uint64_t *comb, const uint64_t *l_scalars,
                                  const uint32_t *key_ids, uint8_t *out32, uint8_t *status, size_t n);
int fourq_keyset_double_mul_bytes_dev(fourq_ctx *ctx, const uint64_t *k_scalars, const uint64_t *comb, const uint64_t *l_scalars,
                                      const uint32_t *key_ids, uint8_t *out32, uint8_t *status, size_t n);
int fourq_keyset_sig_verify(fourq_ctx *ctx, const uint32_t *key_ids, const uint64_t *comb,
                                 const uint8_t *msgs, size_t stride, const uint32_t *lens, size_t msg_len,
                                 const uint8_t *sig64, uint8_t *ok, uint8_t *status, size_t n);
int fourq_keyset_sig_verify_dev(fourq_ctx *ctx, const uint32_t *key_ids, const uint64_t *comb,
                                     const uint8_t *msgs, size_t stride, const uint32_t *lens, size_t msg_len,
                                     const uint8_t *sig64, uint8_t *ok, uint8_t *status, size_t n);

/* ---- bytes to a point: hash to curve (RFC 9380) with SHA-512 XMD, Elligator 2 and the x392 chain on the device -----------------------------
 * RFC 9380's construction instantiated for FourQ.  The suite names FourQ_XMD:SHA-512_ELL2_RO_ and FourQ_XMD:SHA-512_ELL2_NU_ are OURS: no
 * such suite is registered with the RFC or anywhere else, and no other implementation was available to check against -- the yardstick is
 * the CPU restatement tests/h2c_ref.py (hashlib + the oracle's field and point functions) and the fixture made from it with the reference's
 * own point functions (tests/golden/h2c.json).
 *   field      F = GF(p^2), p = 2^127 - 1, elements (re, im), i^2 = -1;  m = 2, k = 128, L = 32
 *   expand_message_xmd (section 5.3.1), H = SHA-512, b_in_bytes = 64, s_in_bytes = 128:
 *              DST_prime = DST || I2OSP(len(DST), 1);  b_0 = H(Z_pad(128 zero bytes) || msg || I2OSP(len_in_bytes, 2) || 0x00 || DST_prime);
 *              b_1 = H(b_0 || 0x01 || DST_prime);  b_2 = H((b_0 xor b_1) || 0x02 || DST_prime);  len_in_bytes = 128 (RO: b_1 || b_2) or
 *              64 (NU: b_1).  DST is 1..FOURQ_H2C_MAX_DST bytes (FOURQ_ERR_INVALID otherwise: no oversize-DST hashing); a HOST pointer in
 *              both flavours, like `table` (it travels in the kernel arguments: nothing is staged, the _dev calls stay capturable).
 *   hash_to_field (section 5.2), count = 2 (RO) or 1 (NU):  e_(i,j) = OS2IP(uniform[32 (j + 2 i) : 32 (j + 2 i) + 32]) mod p, big-endian;
 *              u_i = (e_(i,0), e_(i,1)).
 *   curve      the Montgomery model K t^2 = s^3 + J s^2 + s with J = 2 (a + d) / (a - d), K = 4 / (a - d), a = -1 (appendix D.1):
 *              J = (0x7ffffffffffffc700000000000000509, 0x637a835bf687a14faadcb5733c136818),
 *              K = (0x38ffffffffffffffaf4, 0x1c857ca409785eb055234a8cc3ec97e7);  Z = 2 + i, the first non-square of F in 1 + i, 2 + i, ...
 *              (an element of F is a square iff its norm re^2 + im^2 is a square of GF(p) or zero).  1 + Z u^2 = 0 has no solution.
 *   map_to_curve_elligator2 (section 6.7.1):  x1 = -(J/K) inv0(1 + Z u^2) (-J/K when that is 0);  gx = x^3 + (J/K) x^2 + x / K^2;
 *              x2 = -x1 - J/K;  (x1, sqrt(gx1)) with sgn0 = 1 when gx1 is a square (zero is one), otherwise (x2, sqrt(gx2)) with sgn0 = 0;
 *              (s, t) = (x K, y K).  sgn0 (section 4.1, m = 2) on canonical residues: (re & 1) | ((re == 0) & (im & 1)).
 *   rational map (appendix D.1):  (x, y) = (s / t, (s - 1) / (s + 1)) on -x^2 + y^2 = 1 + d x^2 y^2;  t (s + 1) = 0 gives (0, 1).
 *   RO         P = [392](map(u_0) + map(u_1)), the sum by the complete addition;   NU   P = [392]map(u_0);   x392: curve4q.py:450-455.
 *   output     encode(P) (curve4q.py:41), or canonical affine words.  The neutral point is an ordinary result (01 00 ... 00), as in
 *              fourq_double_mul_*; there is no status.
 * Messages and their rules are those of fourq_sha512_batch: rows of `stride` bytes, lens or msg_len, FOURQ_SIG_MAX_MSG for the host-pointer
 * calls, and the _dev calls clamp a length to `stride` and hash the clamped row.  No branch and no address depends on u or on a message
 * byte (the message may be a password; lengths are public): every selection is a mask, so the same code serves both table-selection
 * modes and fourq_ctx_set_ct_select changes nothing here.  fourq_ctx_reserve covers the one intermediate (u). */
#define FOURQ_H2C_RO 0
#define FOURQ_H2C_NU 1
#define FOURQ_H2C_MAX_DST 255
/* out_u: n x count x 4 words, canonical */
int fourq_hash_to_field_batch(fourq_ctx *ctx, const uint8_t *dst, size_t dst_len, int mode,
                              const uint8_t *msgs, size_t stride, const uint32_t *lens, size_t msg_len, uint64_t *out_u, size_t n);
int fourq_hash_to_field_batch_dev(fourq_ctx *ctx, const uint8_t *dst, size_t dst_len, int mode,
                                  const uint8_t *msgs, size_t stride, const uint32_t *lens, size_t msg_len, uint64_t *out_u, size_t n);
/* u: n x 4 words, each coordinate any value in [0, 2^128); out_affine: the map and the rational map, NO cofactor clearing */
int fourq_map_to_curve_batch(fourq_ctx *ctx, const uint64_t *u, uint64_t *out_affine, size_t n);
int fourq_map_to_curve_batch_dev(fourq_ctx *ctx, const uint64_t *u, uint64_t *out_affine, size_t n);
int fourq_hash_to_curve_batch(fourq_ctx *ctx, const uint8_t *dst, size_t dst_len, int mode,
                              const uint8_t *msgs, size_t stride, const uint32_t *lens, size_t msg_len, uint8_t *out32, size_t n);
int fourq_hash_to_curve_batch_dev(fourq_ctx *ctx, const uint8_t *dst, size_t dst_len, int mode,
                                  const uint8_t *msgs, size_t stride, const uint32_t *lens, size_t msg_len, uint8_t *out32, size_t n);
int fourq_hash_to_curve_affine_batch(fourq_ctx *ctx, const uint8_t *dst, size_t dst_len, int mode,
                                     const uint8_t *msgs, size_t stride, const uint32_t *lens, size_t msg_len, uint64_t *out_affine, size_t n);
int fourq_hash_to_curve_affine_batch_dev(fourq_ctx *ctx, const uint8_t *dst, size_t dst_len, int mode,
                                         const uint8_t *msgs, size_t stride, const uint32_t *lens, size_t msg_len, uint64_t *out_affine, size_t n);

/* ---- oblivious PRF: blind, evaluate, finalize -- what a caller does with a password hashed to a point ---------------------------------------
 * The 2HashDH construction (the core of OPAQUE, Privacy Pass and PSI) on top of "bytes to a point" above.  With G(msg) = hash to curve in
 * RO mode under `dst` as an affine point, N the group order, r the client's blind and k the server's key (scalars: 4 words, ANY value
 * in [0, 2^256), as MUL_endo and DH_endo take them):
 *   blind(msg, r)             out32 = encode(R1toAffine(MUL_endo(r, AffineToR1(G(msg)))))                                     client
 *   evaluate(k, blinded32)    out32 = encode(DH_endo(k, decode(blinded32)))  = fourq_dh_endo_bytes_batch with k on every row  server
 *   finalize(msg, r, ev32)    E = encode(R1toAffine(MUL_endo(1 / r mod N, AffineToR1(decode(ev32)))));  out64 = F(E, msg)     client
 *   eval(k, msg)              out64 = F(encode(DH_endo(k, G(msg))), msg)            the key holder's own evaluation; equals
 *                             finalize(msg, r, evaluate(k, blind(msg, r))) for every r that is not 0 mod N
 *   F(E, msg) = SHA-512(E || msg || "Finalize" || dst || I2OSP(len(dst), 1))        E: 32 bytes
 * Suite.  The suite is this library's own: RFC 9497 registers no FourQ suite, and no other implementation was available to check against;
 * the yardstick is the CPU restatement tests/oprf_ref.py and the fixture tests/golden/oprf.json made with the reference's point functions.
 * Field order of F.  RFC 9497's Finalize hashes I2OSP(len(input), 2) || input || I2OSP(len(E), 2) || E || "Finalize".  Ours puts the
 * fixed-size per-row field first -- it sits in registers as a 32-byte prefix and the row behind it keeps its alignment for vector loads --
 * and the part that is the same for every row last, where it travels by value in the kernel arguments.  The encoding is still injective:
 * the first 32 bytes are E, the LAST byte gives the length of dst and so of the whole tail, and what lies between is msg.
 * Server multiplication.  DH_endo multiplies by 392 k (its cofactor clearing, curve4q.py:446-462): a blinded element with a small-order
 * component is therefore harmless, and the x392 commutes with the blind because G(msg) already lies in the subgroup of order N.
 * Finalize checks nothing beyond decoding, like MUL_*.  There is no RNG in this library: blinds come from the caller, uniformly random
 * in [1, N) for the protocol to hide anything.  The blind and its inverse meet no branch and no address that depends on their value in
 * the inversion (fixed public exponent N - 2, masked selects); in the ladder that holds under fourq_ctx_set_ct_select, as everywhere.
 * Messages and `dst` follow fourq_sha512_batch and fourq_hash_to_curve_batch exactly: rows of `stride` bytes, lens or msg_len,
 * FOURQ_SIG_MAX_MSG on the host-pointer calls (FOURQ_ERR_INVALID above it), the _dev calls clamp a length to `stride`; dst is
 * 1..FOURQ_H2C_MAX_DST bytes and, like `key`, a HOST pointer in both flavours (both travel in kernel arguments: nothing is staged, and
 * after fourq_ctx_reserve(ctx, n) the _dev calls of at most n rows only enqueue and can be captured).  _dev array pointers are 16-byte
 * aligned (status need not be).
 * status, one byte per row; the row of out32 / out64 is all zero unless it is 0.  A bad row never affects its neighbours.
 *   blind      FOURQ_OPRF_BLIND_ZERO when r = 0 (mod N); else FOURQ_SIG_MSG_CLAMPED (_dev only) when the row's length was clamped
 *   evaluate   exactly what fourq_dh_endo_bytes_batch reports (FOURQ_DH_*, FOURQ_BYTES_DECODE_BASE + FOURQ_DECODE_*)
 *   finalize   FOURQ_BYTES_DECODE_BASE + FOURQ_DECODE_* when ev32 does not decode; else FOURQ_OPRF_BLIND_ZERO; else FOURQ_SIG_MSG_CLAMPED
 *   eval       FOURQ_DH_NEUTRAL when k = 0 (mod N); else FOURQ_SIG_MSG_CLAMPED
 * Work buffer: each call's intermediates (work_layout.h, Oprf*) stay below the signature check's, so fourq_ctx_reserve does not grow. */
#define FOURQ_OPRF_BLIND_ZERO 48      /* status: the blind is 0 mod N (it has no inverse; [0]G is the neutral point for every msg) */
int fourq_oprf_blind_batch(fourq_ctx *ctx, const uint8_t *dst, size_t dst_len, const uint8_t *msgs, size_t stride, const uint32_t *lens,
                           size_t msg_len, const uint64_t *blinds, uint8_t *out32, uint8_t *status, size_t n);
int fourq_oprf_blind_batch_dev(fourq_ctx *ctx, const uint8_t *dst, size_t dst_len, const uint8_t *msgs, size_t stride, const uint32_t *lens,
                               size_t msg_len, const uint64_t *blinds, uint8_t *out32, uint8_t *status, size_t n);
/* key: HOST pointer, 4 words, one key for the whole batch */
int fourq_oprf_evaluate_batch(fourq_ctx *ctx, const uint64_t *key, const uint8_t *blinded32, uint8_t *out32, uint8_t *status, size_t n);
int fourq_oprf_evaluate_batch_dev(fourq_ctx *ctx, const uint64_t *key, const uint8_t *blinded32, uint8_t *out32, uint8_t *status, size_t n);
int fourq_oprf_finalize_batch(fourq_ctx *ctx, const uint8_t *dst, size_t dst_len, const uint8_t *msgs, size_t stride, const uint32_t *lens,
                              size_t msg_len, const uint64_t *blinds, const uint8_t *evaluated32, uint8_t *out64, uint8_t *status, size_t n);
int fourq_oprf_finalize_batch_dev(fourq_ctx *ctx, const uint8_t *dst, size_t dst_len, const uint8_t *msgs, size_t stride, const uint32_t *lens,
                                  size_t msg_len, const uint64_t *blinds, const uint8_t *evaluated32, uint8_t *out64, uint8_t *status, size_t n);
int fourq_oprf_eval_batch(fourq_ctx *ctx, const uint64_t *key, const uint8_t *dst, size_t dst_len, const uint8_t *msgs, size_t stride,
                          const uint32_t *lens, size_t msg_len, uint8_t *out64, uint8_t *status, size_t n);
int fourq_oprf_eval_batch_dev(fourq_ctx *ctx, const uint64_t *key, const uint8_t *dst, size_t dst_len, const uint8_t *msgs, size_t stride,
                              const uint32_t *lens, size_t msg_len, uint8_t *out64, uint8_t *status, size_t n);
/* out[i] = 1 / scalars[i] mod N, n x 4 words in and out, canonical; scalars: ANY value in [0, 2^256).  No status: a scalar that is
 * 0 mod N gives 0 (and touches no neighbour, although one Fermat chain a^(N-2) serves up to 16 elements: Montgomery's trick inside a lane). */
int fourq_scalar_inv_batch(fourq_ctx *ctx, const uint64_t *scalars, uint64_t *out, size_t n);
int fourq_scalar_inv_batch_dev(fourq_ctx *ctx, const uint64_t *scalars, uint64_t *out, size_t n);
/* TEST HOOK: k = 1, 8 or 16 elements per Fermat chain in fourq_scalar_inv_* and fourq_oprf_finalize_* whatever the batch size, 0 = chosen
 * by batch size again (results do not depend on it).  FOURQ_ERR_INVALID unless the process runs with FOURQ_DEBUG_ROUTES=1. */
int fourq_ctx_set_scinv_group(fourq_ctx *ctx, int k);

/* ---- oblivious PRF: proofs -- a batched Chaum-Pedersen (DLEQ) proof that a batch was evaluated with the key behind a public key -----------------
 * What a VERIFIABLE oblivious PRF adds (RFC 9497 section 2.2, the shape Privacy Pass uses): the server proves that every evaluated element
 * of a group is the blinded one multiplied by the key of its published public key, without showing the key.  groups x group_size rows laid
 * out group after group, as fourq_msm_*; ONE proof per group, so a server answers many small requests (down to one row per proof) in one call.
 * Suite.  Like the OPRF's, the suite is this library's own (RFC 9497 registers none for FourQ); the yardstick is the CPU restatement
 * tests/dleq_ref.py and the fixture tests/golden/dleq.json made with the reference's point functions.
 * Notation.  Gen = (Gx, Gy) the generator, N the group order, k the server's key (4 words, any value in [0, 2^256)), K = 392 k mod N the
 * scalar DH_endo really multiplies by (its cofactor clearing, curve4q.py:446-462: evaluated = [K]blinded), H = SHA-512, LE(x) the
 * little-endian integer of a byte string, dst 1..FOURQ_H2C_MAX_DST bytes, tail(L) = L || dst || I2OSP(len(dst), 1) (the shape of F's tail).
 *   public key   pk32 = encode(DH_endo(k, Gen)): what fourq_oprf_evaluate_batch returns for the one row encode(Gen)
 *   rows         row i = (g, j), j < group_size:  C_i = blinded32[i], D_i = evaluated32[i], 32-byte encodings
 *   d_i          = LE(H(pk32 || C_i || D_i || I2OSP(j, 4) || tail("Composite"))) mod N: 100 fixed bytes, then the tail; j is the index
 *                INSIDE the group, so a group's proof does not depend on where in the batch the group stands
 *   composites   M_g = sum_j [d_gj]decode(C_gj);  verifier: Z_g = sum_j [d_gj]decode(D_gj);  prover: Z_g = DH_endo(k, M_g) -- one
 *                multiplication per group: the prover hashes D and never decodes it.  M32 = encode(M_g), Z32 = encode(Z_g).
 *   prove        r = nonces[g] mod N (from the caller, like the blinds: there is no RNG in this library; uniformly random, never reused);
 *                t2 = encode([r]Gen);  t3 = encode(R1toAffine(MUL_endo(r, AffineToR1(M_g))));
 *                c = LE(H(pk32 || M32 || Z32 || t2 || t3 || tail("Challenge"))) mod N;  s = (r - c K) mod N;  proof64[g] = LE32(c) || LE32(s)
 *   verify       t2' = encode([s]Gen + [c]decode(pk32))   (fourq_double_mul_bytes_batch with pk32 on every group's row);
 *                t3' = encode([s]M_g + [c]Z_g)            (fourq_msm_bytes_batch over the groups of two (s, M32), (c, Z32));
 *                ok[g] = (LE(H(pk32 || M32 || Z32 || t2' || t3' || tail("Challenge"))) mod N == c)
 * status, one byte per group; the group's output row is all zero, and ok is 0, unless it is 0.  A bad group never affects another.
 *   prove        FOURQ_BYTES_DECODE_BASE + the LARGEST FOURQ_DECODE_* among the group's C rows; else FOURQ_DH_NEUTRAL when k = 0 (mod N);
 *                else FOURQ_DLEQ_NONCE_ZERO when r = 0 (mod N).  An evaluated row that does not decode does not stop the prover.
 *   verify       FOURQ_BYTES_DECODE_BASE + the largest decode code among the group's C and D rows and pk32 (a pk32 that does not decode
 *                marks every group); else FOURQ_SIG_S_RANGE when LE(c) >= N or LE(s) >= N; else 0, and ok is the comparison.
 *   composites   the decode part of verify's, without pk32 (it is only hashed there); M32 and Z32 are both zero unless it is 0.
 *   A composite that comes out as the NEUTRAL point is refused by the next stage's decode, FOURQ_BYTES_DECODE_BASE +
 *   FOURQ_DECODE_REF_ATTRIBUTE_ERROR (prove, verify; composites hands out its encoding 01 00 .. 00): it takes an accident of the kind of a
 *   hash collision -- or blinded elements outside the subgroup of order N, for which DH_endo may also report FOURQ_DH_NEUTRAL.
 * Secrets.  k, K and r meet no branch and no address that depends on their value in the proofs' own kernels (reductions, one product, the
 * mul-sub, masked statuses); in the ladders and the comb that holds under fourq_ctx_set_ct_select, as everywhere.  d, M, Z and c are public.
 * Arguments.  `key`, `pk32` and `dst` are HOST pointers in both flavours (they travel in kernel arguments); `comb` is the generator's comb
 * or NULL = the staged one, as in fourq_sig_*.  groups == 0: FOURQ_OK, nothing touched.  group_size == 0 with groups > 0, or groups *
 * group_size (overflow-checked) above FOURQ_MAX_BATCH -- for verify and reserve also 2 * groups, the rows of its sum of two --:
 * FOURQ_ERR_INVALID.  _dev array pointers are 16-byte aligned (ok and status need not be); nothing is staged before the arguments are accepted.
 * Work buffer.  The inner calls carve their own layouts; this call's regions lie behind the largest of them (dleq_layout.h), which is MORE
 * than fourq_ctx_reserve sizes: fourq_dleq_reserve(groups, group_size) is the reservation for these calls.  After it a _dev call of at
 * most that shape allocates and synchronises nothing and, with the comb staged, can be captured.  The host-array calls are synchronous --
 * copy in, the _dev call, copy out -- without chunks, as fourq_msm_*: the outputs are per group.
 * Cost (not measured into this text; profiles/dleq_timing.txt): prove is one decode + ladder per row and three multiplications per group
 * (comb, DH_endo, MUL_endo); verify two per row and four per group ([s]G + [c]pk counts two, the sum of two counts two). */
#define FOURQ_DLEQ_NONCE_ZERO 80      /* status of prove: the nonce is 0 mod N (s would be -c K: the proof would hand out the key) */
int fourq_dleq_reserve(fourq_ctx *ctx, size_t groups, size_t group_size);
/* the verifier's composites: m32, z32 groups x 32 bytes */
int fourq_dleq_composites(fourq_ctx *ctx, const uint8_t *dst, size_t dst_len, const uint8_t *pk32, const uint8_t *blinded32,
                          const uint8_t *evaluated32, uint8_t *m32, uint8_t *z32, uint8_t *status, size_t groups, size_t group_size);
int fourq_dleq_composites_dev(fourq_ctx *ctx, const uint8_t *dst, size_t dst_len, const uint8_t *pk32, const uint8_t *blinded32,
                              const uint8_t *evaluated32, uint8_t *m32, uint8_t *z32, uint8_t *status, size_t groups, size_t group_size);
/* nonces: groups x 4 words; proof64: groups x 64 bytes */
int fourq_dleq_prove(fourq_ctx *ctx, const uint64_t *key, const uint64_t *comb, const uint8_t *dst, size_t dst_len, const uint8_t *blinded32,
                     const uint8_t *evaluated32, const uint64_t *nonces, uint8_t *proof64, uint8_t *status, size_t groups, size_t group_size);
int fourq_dleq_prove_dev(fourq_ctx *ctx, const uint64_t *key, const uint64_t *comb, const uint8_t *dst, size_t dst_len, const uint8_t *blinded32,
                         const uint8_t *evaluated32, const uint64_t *nonces, uint8_t *proof64, uint8_t *status, size_t groups, size_t group_size);
int fourq_dleq_verify(fourq_ctx *ctx, const uint8_t *pk32, const uint64_t *comb, const uint8_t *dst, size_t dst_len, const uint8_t *blinded32,
                      const uint8_t *evaluated32, const uint8_t *proof64, uint8_t *ok, uint8_t *status, size_t groups, size_t group_size);
int fourq_dleq_verify_dev(fourq_ctx *ctx, const uint8_t *pk32, const uint64_t *comb, const uint8_t *dst, size_t dst_len, const uint8_t *blinded32,
                          const uint8_t *evaluated32, const uint8_t *proof64, uint8_t *ok, uint8_t *status, size_t groups, size_t group_size);

/* ---- verifiable random function: prove, verify and proof-to-hash in batches, under the signature scheme's keys ---------------------------------
 * What leader election and sortition over a validator set, verifiable lotteries and authenticated denial ask for: the key holder maps a
 * public input alpha to a pseudorandom output beta and a proof; everyone else checks the proof and gets the same beta from it.  One row
 * per (key, alpha); rows are independent.
 * Suite.  The suite is this library's own, as the OPRF's and the DLEQ's are: its structure is that of ECVRF (RFC 9381) with Elligator 2;
 * interoperability with anything else is NOT claimed.  The yardstick is the CPU restatement tests/vrf_ref.py and the fixture
 * tests/golden/vrf.json made with the reference's point functions.
 * Notation.  H = SHA-512, LE(x) the little-endian integer of a byte string, G the generator, N the group order, dst 1..FOURQ_H2C_MAX_DST
 * bytes, tail(L) = L || dst || I2OSP(len(dst), 1) as in fourq_dleq_*, INV392 = 1 / 392 mod N.  Keys are fourq_sig_*'s, so one key pair
 * serves signing and the VRF: k = H(sk32), x = LE(k[0:32]) (unreduced), pk32 = fourq_sig_keygen_batch(sk32).  alpha is the row's message,
 * under the rules fourq_sig_* has for `stride`, `lens`, `msg_len` and FOURQ_SIG_MAX_MSG.
 *   Hpt      = hash to curve, RO mode, under dst, of the string pk32 || alpha (affine, in the subgroup of order N);  h32 = encode(Hpt)
 *   prove(sk32, pk32, alpha) -> proof96
 *     Gamma  = R1toAffine(MUL_endo(x, AffineToR1(Hpt)));  gamma32 = encode(Gamma)
 *     r      = LE(H(k[32:64] || h32)) mod N                  (64 bytes hashed: deterministic, no RNG, no nonce from the caller)
 *     u32    = encode([r]G) (the comb);  v32 = encode(R1toAffine(MUL_endo(r, AffineToR1(Hpt))))
 *     c      = LE(H(pk32 || h32 || gamma32 || u32 || v32 || tail("VrfVerify"))) mod N        (160 fixed bytes, then the tail)
 *     s      = (r - c x) mod N;  proof96 = gamma32 || LE32(c) || LE32(s)
 *     pk32 is an input, as in fourq_sig_sign_batch: neither derived again nor checked against sk32.
 *   verify(pk32, alpha, proof96) -> ok, status, beta64
 *     Y      = decode(pk32);  Gamma = decode(proof96[0:32]);  c, s = LE(proof96[32:64]), LE(proof96[64:96])
 *     W      = [392]Gamma by the x392 chain (curve4q.py:450-455, FOURQ_PT_COFACTOR392);  w32 = encode(W)
 *     u32'   = encode([s]G + [c]Y)                     (fourq_double_mul_bytes_batch with k = s, l = c)
 *     v32'   = encode([s]Hpt + [c INV392 mod N]W)      (fourq_msm_bytes_batch over the groups of two (s, h32), (c INV392 mod N, w32))
 *     ok     = (LE(H(pk32 || h32 || proof96[0:32] || u32' || v32' || tail("VrfVerify"))) mod N == c)
 *     beta64 = H(w32 || tail("VrfOutput")) when ok, else 64 zero bytes
 *   proof_to_hash(proof96) -> beta64 = H(encode([392]decode(proof96[0:32])) || tail("VrfOutput"));  c and s are not looked at
 * The label "VrfVerify" differs from the DLEQ's "Challenge" on purpose: both prefixes are 160 bytes of five encodings, and a VRF proof must
 * not double as an OPRF proof under the same dst.
 * Why W and INV392.  Gamma comes from the prover, who is the adversary for uniqueness, and MUL_endo is not [k]P outside the subgroup of
 * order N.  So the verifier never feeds Gamma to a ladder: it clears the cofactor first and divides the challenge by 392 to compensate
 * ([c INV392]W = [c]Gamma for an honest Gamma).  The output hashes W, not Gamma, so a torsion component of Gamma cannot change beta: a
 * prover who shifts Gamma by a point of order 7 or 14 and hashes the challenge again is accepted, with the same beta.
 * pk32 is NOT checked for order N by fourq_vrf_verify, exactly as fourq_sig_verify_batch does not check it; callers who need uniqueness
 * against adversarially generated keys use fourq_vrf_verify_keyed: registration checks the order.
 * fourq_vrf_verify_keyed[_dev]: the keys named by their index in the set of fourq_keyset_set.  Every hash reads the key bytes exactly as
 * registered, u32' goes through fourq_keyset_double_mul_bytes_dev, and for an accepted key beta64, ok and status equal fourq_vrf_verify on
 * pk32[i] = key[id_i] byte for byte.  With constant-time selection the rows' key bytes are gathered by index and the unkeyed route runs on
 * them, as in fourq_keyset_sig_verify; the answers are identical in both modes.
 * status, one byte per row; verify's ok is 0 and beta64 all zero unless it is 0.  A bad row never affects another.  Verify, in this order
 * of precedence:
 *     FOURQ_KEYSET_ID_RANGE, then the key's own status   (the keyed call only, exactly as fourq_keyset_sig_verify orders them; the host
 *                                                         flavour refuses an index outside the set with FOURQ_ERR_INVALID, the _dev
 *                                                         flavour clamps it before it becomes an address)
 *     FOURQ_BYTES_DECODE_BASE + FOURQ_DECODE_* of pk32
 *     the same code of gamma32
 *     FOURQ_SIG_MSG_CLAMPED                              (_dev only)
 *     FOURQ_SIG_S_RANGE                                  LE(c) >= N or LE(s) >= N
 *     FOURQ_VRF_GAMMA_NEUTRAL                            W is the neutral point: Gamma has no component of order N
 *   proof_to_hash reports the code of gamma32 and FOURQ_VRF_GAMMA_NEUTRAL only.  prove has no status, like fourq_sig_sign_batch; its _dev
 *   flavour hashes a clamped row; x = 0 or r = 0 (mod N) would take a SHA-512 preimage and has no code.  An Hpt that is the neutral point
 *   takes a hash accident: the sum of two refuses its encoding (FOURQ_BYTES_DECODE_BASE + FOURQ_DECODE_REF_ATTRIBUTE_ERROR, last in order).
 * Secrets.  k, x and r meet no branch and no address that depends on their value in the VRF's own kernels (one reduction, the mul-sub);
 * in the ladders and the comb that holds under fourq_ctx_set_ct_select, as everywhere.  h32, Gamma, c and s are public.
 * Arguments.  `dst` is a HOST pointer in both flavours; `comb` is the generator's comb, or NULL = the staged one.  n == 0: FOURQ_OK,
 * nothing touched.  FOURQ_ERR_INVALID: a NULL array, a dst of 0 or more than FOURQ_H2C_MAX_DST bytes, n above FOURQ_MAX_BATCH -- for
 * verify and reserve above FOURQ_MAX_BATCH / 2, its sum of two has 2 n rows --, the keyed call with no set installed.  _dev array pointers
 * are 16-byte aligned (ok and status need not be).
 * Work buffer.  The inner calls carve their own layouts; this call's regions lie behind the largest of them (vrf_layout.h), which is more
 * than fourq_ctx_reserve sizes: fourq_vrf_reserve(ctx, n) is the reservation.  After it, with the comb staged, a _dev call of at most n
 * rows allocates nothing and synchronises nothing.  The host-pointer calls run the chunked pipeline: copy in, the _dev call, copy out.
 * Names.  The entry points carry no _batch, as fourq_keyset_sig_verify does not: names ending in _batch belong to the per-element calls
 * whose argument contract one table enumerates.  The keyed call is fourq_vrf_verify_keyed, not fourq_keyset_*: that prefix names the
 * calls of the key set's own section.
 * Cost: tools/vrf_timing.py measures verify against the sum of its inner calls, keyed against unkeyed, and prove
 * (profiles/vrf_timing.txt); nothing of it is quoted here. */
#define FOURQ_VRF_GAMMA_NEUTRAL 128   /* status of verify and proof_to_hash: [392]Gamma is the neutral point */
int fourq_vrf_reserve(fourq_ctx *ctx, size_t n);
/* sk32, pk32: n x 32 bytes; proof96: n x 96 bytes */
int fourq_vrf_prove(fourq_ctx *ctx, const uint8_t *sk32, const uint8_t *pk32, const uint64_t *comb, const uint8_t *dst, size_t dst_len,
                    const uint8_t *msgs, size_t stride, const uint32_t *lens, size_t msg_len, uint8_t *proof96, size_t n);
int fourq_vrf_prove_dev(fourq_ctx *ctx, const uint8_t *sk32, const uint8_t *pk32, const uint64_t *comb, const uint8_t *dst, size_t dst_len,
                        const uint8_t *msgs, size_t stride, const uint32_t *lens, size_t msg_len, uint8_t *proof96, size_t n);
/* beta64: n x 64 bytes */
int fourq_vrf_verify(fourq_ctx *ctx, const uint8_t *pk32, const uint64_t *comb, const uint8_t *dst, size_t dst_len,
                     const uint8_t *msgs, size_t stride, const uint32_t *lens, size_t msg_len,
                     const uint8_t *proof96, uint8_t *beta64, uint8_t *ok, uint8_t *status, size_t n);
int fourq_vrf_verify_dev(fourq_ctx *ctx, const uint8_t *pk32, const uint64_t *comb, const uint8_t *dst, size_t dst_len,
                         const uint8_t *msgs, size_t stride, const uint32_t *lens, size_t msg_len,
                         const uint8_t *proof96, uint8_t *beta64, uint8_t *ok, uint8_t *status, size_t n);
int fourq_vrf_verify_keyed(fourq_ctx *ctx, const uint32_t *key_ids, const uint64_t *comb, const uint8_t *dst, size_t dst_len,
                            const uint8_t *msgs, size_t stride, const uint32_t *lens, size_t msg_len,
                            const uint8_t *proof96, uint8_t *beta64, uint8_t *ok, uint8_t *status, size_t n);
int fourq_vrf_verify_keyed_dev(fourq_ctx *ctx, const uint32_t *key_ids, const uint64_t *comb, const uint8_t *dst, size_t dst_len,
                                const uint8_t *msgs, size_t stride, const uint32_t *lens, size_t msg_len,
                                const uint8_t *proof96, uint8_t *beta64, uint8_t *ok, uint8_t *status, size_t n);
int fourq_vrf_proof_to_hash(fourq_ctx *ctx, const uint8_t *dst, size_t dst_len, const uint8_t *proof96, uint8_t *beta64, uint8_t *status, size_t n);
int fourq_vrf_proof_to_hash_dev(fourq_ctx *ctx, const uint8_t *dst, size_t dst_len, const uint8_t *proof96, uint8_t *beta64, uint8_t *status, size_t n);

/* ---- threshold sharing: Shamir shares modulo N, Feldman commitments and their check, Lagrange coefficients, combination ----------------------
 * For a key that is split t-of-n across machines.  N is the group order; scalars are 4 little-endian words.  A party's identifier is a
 * uint32_t id, the evaluation point x = id; ids are public.  The id 0 is refused: f(0) is the secret.  A polynomial is t coefficients
 * a_0 .. a_(t-1), each ANY value in [0, 2^256), read modulo N; a_0 is the secret; 1 <= t <= FOURQ_SHAMIR_MAX_T.
 * Party-major layout: wherever an array holds one 32-byte item per (party, row), block i holds party i's n rows contiguously, item (i, r)
 * at index i * n + r -- what a dealer sends to party i, what a client receives from server i.  No call asks the caller to interleave.
 *   shares          shares[p][r] = sum_j a_rj ids[p]^j mod N, canonical.  coeffs: n x t x 4 words, row r's coefficients together; ids: m;
 *                   shares: party-major m x n x 4 words.  status[p]: FOURQ_SHAMIR_ID_ZERO where ids[p] == 0 (block p is all zero), else 0.
 *                   Repeated ids are no error here: equal blocks.  One (party, row) per lane, Horner's rule from a_(t-1) down.
 *   lagrange        lambda[set][i] = prod_(j != i) x_j / (x_j - x_i) mod N, canonical: the coefficients at 0.  ids: sets x t.  status[set]:
 *                   FOURQ_SHAMIR_ID_ZERO if any id of the set is 0, else FOURQ_SHAMIR_ID_REPEATED if two are equal, else 0.  A set with
 *                   a status has ALL its rows zero; other sets are unaffected.  t = 1 gives lambda = 1.
 *   combine         out[r] = sum_i lambda_i shares[i][r] mod N for ONE set of t ids; shares: party-major t x n x 4 words, each any value
 *                   in [0, 2^256).  status: ONE byte, lagrange's codes; non-zero: every out row is zero.
 *   combine_points  out32[r] = encode(sum_i [lambda_i]decode(points32[i][r])) for ONE set of t ids; points32: party-major t x n x 32 bytes;
 *                   status: n bytes.  out32 and status are byte for byte what fourq_msm_bytes_batch returns for groups = n, group_size = t,
 *                   scalar row (r, i) = lambda_i and point row (r, i) = points32[i][r]: 16 + the largest FOURQ_DECODE_* of a group with its
 *                   zero row, the neutral point as an ordinary result.  A bad id set marks EVERY row with its code and zeroes it, ahead
 *                   of the decode codes.  "In the exponent": with points32[i] = server i's fourq_oprf_evaluate_batch reply under its
 *                   share, out32 is the reply under the undivided key, byte for byte.
 *   public_shares   out32[g] = encode(sum_j [ids[g]^j mod N]decode(C_gj)): party ids[g]'s verification share from the Feldman
 *                   commitments C_g0 .. C_g,t-1 of polynomial g (commits32: groups x t x 32 bytes; C_gj = encode([a_gj]G): the comb over
 *                   the coefficients, then fourq_encode_batch).  status: fourq_msm_bytes_batch's per group, or FOURQ_SHAMIR_ID_ZERO,
 *                   which comes first and zeroes the row.  A coefficient that is 0 mod N has the commitment 01 00 .. 00, the neutral
 *                   point's encoding, which the reference's decode refuses: as in fourq_msm_bytes_batch that group reports
 *                   16 + FOURQ_DECODE_REF_ATTRIBUTE_ERROR.  A dealer draws its coefficients from [1, N).
 *   verify          ok[g] = (public_share_g == encode([shares[g]]G)); shares: groups x 4 words; the right side through the generator's comb
 *                   (`comb`, or NULL = the staged one, as fourq_sig_*) and encode.  status: that of public_shares, else
 *                   FOURQ_SIG_S_RANGE where shares[g] >= N; ok is 0 wherever the status is not.  Both sides may be the neutral point
 *                   (f(x) = 0 mod N): that compares equal, with status 0.
 * Secrets.  Coefficients, shares and combine's out never steer a branch or an address: straight-line code on whole words (shamir.hip.h,
 * scalar_n.hip.h).  Ids, lambda, commitments and verification shares are public.  The library has no random numbers: coefficients come
 * from the caller.
 * Arguments.  groups, n, sets or m == 0: FOURQ_OK, nothing touched.  t == 0 with work to do, t > FOURQ_SHAMIR_MAX_T, a NULL array, a
 * misaligned _dev pointer, or n x t (shares: also m x n) above FOURQ_MAX_BATCH: FOURQ_ERR_INVALID before anything is staged.  Every _dev
 * array is 16-byte aligned except ok and status.
 * Work buffer.  combine_points, public_shares and verify run fourq_msm_bytes_batch_dev (and verify the comb) as inner calls; their own
 * regions lie behind the largest inner layout (shamir_layout.h).  fourq_shamir_reserve(ctx, rows, t) sizes the buffers for any call of
 * this section with at most rows x t items (shares needs none); after it, with the comb staged, a _dev call allocates nothing,
 * synchronises nothing and can be captured.  The host flavours copy in, run the twin and copy out, in one piece.
 * Names: no _batch, as the VRF's.  Cost: tools/shamir_timing.py (profiles/shamir_timing.txt); nothing of it is quoted here. */
#define FOURQ_SHAMIR_MAX_T 4096
#define FOURQ_SHAMIR_ID_ZERO 144      /* status: the id is 0 (f(0) is the secret) */
#define FOURQ_SHAMIR_ID_REPEATED 160  /* status of lagrange and the combines: two ids of the set are equal */
int fourq_shamir_reserve(fourq_ctx *ctx, size_t rows, size_t t);
int fourq_shamir_shares(fourq_ctx *ctx, const uint64_t *coeffs, const uint32_t *ids, uint64_t *shares, uint8_t *status, size_t n, size_t t, size_t m);
int fourq_shamir_shares_dev(fourq_ctx *ctx, const uint64_t *coeffs, const uint32_t *ids, uint64_t *shares, uint8_t *status, size_t n, size_t t, size_t m);
int fourq_shamir_lagrange(fourq_ctx *ctx, const uint32_t *ids, uint64_t *lambda, uint8_t *status, size_t sets, size_t t);
int fourq_shamir_lagrange_dev(fourq_ctx *ctx, const uint32_t *ids, uint64_t *lambda, uint8_t *status, size_t sets, size_t t);
int fourq_shamir_combine(fourq_ctx *ctx, const uint32_t *ids, const uint64_t *shares, uint64_t *out, uint8_t *status, size_t n, size_t t);
int fourq_shamir_combine_dev(fourq_ctx *ctx, const uint32_t *ids, const uint64_t *shares, uint64_t *out, uint8_t *status, size_t n, size_t t);
int fourq_shamir_combine_points(fourq_ctx *ctx, const uint32_t *ids, const uint8_t *points32, uint8_t *out32, uint8_t *status, size_t n, size_t t);
int fourq_shamir_combine_points_dev(fourq_ctx *ctx, const uint32_t *ids, const uint8_t *points32, uint8_t *out32, uint8_t *status, size_t n, size_t t);
int fourq_shamir_public_shares(fourq_ctx *ctx, const uint8_t *commits32, const uint32_t *ids, uint8_t *out32, uint8_t *status, size_t groups, size_t t);
int fourq_shamir_public_shares_dev(fourq_ctx *ctx, const uint8_t *commits32, const uint32_t *ids, uint8_t *out32, uint8_t *status, size_t groups, size_t t);
int fourq_shamir_verify(fourq_ctx *ctx, const uint64_t *comb, const uint8_t *commits32, const uint32_t *ids, const uint64_t *shares,
                        uint8_t *ok, uint8_t *status, size_t groups, size_t t);
int fourq_shamir_verify_dev(fourq_ctx *ctx, const uint64_t *comb, const uint8_t *commits32, const uint32_t *ids, const uint64_t *shares,
                            uint8_t *ok, uint8_t *status, size_t groups, size_t t);

/* ---- primitives (one reference function per op, batched) --------------------------------------
 * Used by the Python mirror of the reference's helper API (GFp.*, GFp2.*, DBL, ADD, phi, ...) and by
 * the parity tests to check every layer of the path on the GPU.  in/out are HOST pointers;
 * element strides are fourq_prim_words(). */
enum fourq_prim {
    /* GFp, fields.py:29-106: in = a[2] b[2] */
    FOURQ_FP_ADD = 0, FOURQ_FP_SUB = 1, FOURQ_FP_MUL = 2, FOURQ_FP_SQR = 3, FOURQ_FP_NEG = 4, FOURQ_FP_INV = 5,
    FOURQ_FP_INVSQRT = 6,       /* fields.py:110 */
    /* GFp.select(c, x, y) fields.py:59-64, GFp2.select fields.py:236-238: in = c[2] x y; raw 128-bit words,
     * y ^ ((mask * c) & (x ^ y)) with the reference's mask = 2^512 - 1, no reduction (as the reference) */
    FOURQ_FP_SELECT = 7, FOURQ_FP2_SELECT = 23,
    /* GFp2, fields.py:156-199: in = a[4] b[4] */
    FOURQ_FP2_ADD = 16, FOURQ_FP2_SUB = 17, FOURQ_FP2_MUL = 18, FOURQ_FP2_SQR = 19, FOURQ_FP2_NEG = 20,
    FOURQ_FP2_CONJ = 21, FOURQ_FP2_INV = 22,
    /* curve4q.py:100-175 */
    FOURQ_PT_DBL = 32,          /* R1[20] -> R1[20] */
    FOURQ_PT_ADD = 33,          /* R1[20] R2[16] -> R1[20] */
    FOURQ_PT_ADD_CORE = 34,     /* R3[16] R2[16] -> R1[20] */
    FOURQ_PT_R1TOR2 = 35,       /* R1[20] -> R2[16] */
    FOURQ_PT_R1TOR3 = 36,       /* R1[20] -> R3[16] */
    FOURQ_PT_R2TOR4 = 37,       /* R2[16] -> R4[12] */
    /* curve4q.py:258-322 */
    FOURQ_PT_TAU = 38,          /* (X,Y,Z)[12] -> [12] */
    FOURQ_PT_TAU_DUAL = 39,     /* [12] -> R1[20] */
    FOURQ_PT_UPSILON = 40,      /* [12] -> [12] */
    FOURQ_PT_CHI = 41,          /* [12] -> [12] */
    FOURQ_PT_PHI = 42,          /* R1[20] -> R1[20] */
    FOURQ_PT_PSI = 43,          /* R1[20] -> R1[20] */
    FOURQ_PT_ON_CURVE = 44,     /* affine[8] -> [1] (0/1)            curve4q.py:23 */
    FOURQ_PT_COFACTOR392 = 45,  /* affine[8] -> R1[20]               curve4q.py:450-455 */
    FOURQ_PT_R1TOAFFINE = 46,   /* R1[20] -> affine[8]               curve4q.py:103 */
    FOURQ_PT_MAP_ELL2 = 47,     /* u[4] -> affine[8]: Elligator 2 + the rational map ("bytes to a point" above) */
    /* curve4q.py:216-226, :339-380 */
    FOURQ_SC_DECOMPOSE = 64,    /* m[4] -> a1..a4 [4] */
    FOURQ_SC_RECODE = 65,       /* v[4] = decompose(m) -> [5]: sign bits 0..63, digit bit-planes 0,1,2, digit 64 */
    FOURQ_SC_WINDOWED = 66,     /* m[4] -> [8]: 63 bytes, byte i = (sgn[i] << 3) | ind[i] */
    /* arithmetic modulo N (scalar_n.hip.h): inputs ANY value of their width, outputs canonical in [0, N) */
    FOURQ_SC_REDUCE512 = 67,    /* x[8] -> [4]: x mod N */
    FOURQ_SC_MULSUB = 68,       /* r[4] a[4] h[4] -> [4]: (r - a h) mod N */
    FOURQ_SC_MUL = 69,          /* a[4] b[4] -> [4]: a b mod N */
    /* the digits of FOURQ_SC_RECODE as the fused ladders read them: step i (0..63) is nibble i % 8 of word i / 8, bits 0..2 the digit,
     * bit 3 set when the step subtracts (sign bit 0) */
    FOURQ_SC_RECODE_NIBBLES = 70, /* v[4] = decompose(m) -> [9]: the eight 32-bit words, one per output word, then digit 64 */
    FOURQ_SC_INV = 71           /* a[4] -> [4]: 1 / a mod N, canonical; 0 when a = 0 (mod N) */
};
int fourq_prim_words(int op, size_t *in_words, size_t *out_words);
int fourq_prim_batch(fourq_ctx *ctx, int op, const uint64_t *in, uint64_t *out, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* FOURQ_AMD_H */
