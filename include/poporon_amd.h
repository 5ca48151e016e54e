/*
 * poporon_amd.h -- batch extension of the poporon C API for MI355X.
 *
 * The reference has no batch API: callers loop poporon_encode/poporon_decode
 * one codeword at a time (include/poporon.h:90-91, src/encode.c:236-252,
 * src/decode.c:596-612).  These entry points take many codewords at once
 * behind the same handle.  Each per-codeword result equals what the
 * single-codeword call would return for that codeword (bytes, bool and
 * corrected_num), see tests/test_gpu_parity.py.
 *
 * Layout: codeword c's message is data[c*data_stride .. +size), its parity
 * parity[c*parity_stride .. +num_roots).  Strides and base pointers may have
 * any alignment; 4-byte aligned strides/bases take the fast load path.
 *
 * Device variants take device pointers (hipMalloc'd or any HIP-visible
 * allocation, e.g. a torch tensor's data_ptr()) and enqueue asynchronously on
 * `stream` (a hipStream_t; NULL = the null stream).  Host variants copy
 * through pinned staging in chunks and return when the results are in host
 * memory.  A handle is not reentrant (same rule as the reference handle).
 *
 * The batch calls serve RS handles and BCH handles (PPLN_FEC_BCH, symbol_size
 * 3..5): for BCH, `size` is the message byte count (>= the info byte image),
 * parity rows hold the parity byte image, and there are no erasure or
 * external-syndrome variants; d_corrected[c] = 0 where d_ok[c] = 0.
 *
 * LDPC handles (PPLN_FEC_LDPC) have batch calls of their own, poporon_ldpc_*
 * below: their encode rewrites the data, their iteration counts do not fit a
 * byte and their soft decode takes a third input.  The RS / BCH batch calls
 * return false with a message on an LDPC handle.
 *
 * Every entry point returns false and records a message (poporon_amd_last_error)
 * on invalid arguments, an unsupported configuration, or a HIP failure.  There
 * is no CPU fallback: without a usable GPU these calls fail.
 */
#ifndef POPORON_AMD_H
#define POPORON_AMD_H

#include <stddef.h>
#include <stdint.h>

#include "poporon.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Message for the last failing call on this thread ("" if none). */
const char *poporon_amd_last_error(void);

/* poporon_decode (RS) writes this to *corrected_num (and the handle's
 * last_corrected) when the call failed on the device side -- no usable GPU,
 * or a HIP error -- rather than on the codeword: the reference never reports
 * more than num_roots corrections, so a drop-in caller tells "device error"
 * from "uncorrectable" (false with 0..num_roots) without a new entry point. */
#define POPORON_AMD_DEVICE_ERROR ((size_t)-1)

/* Number of HIP devices visible (0 when no GPU / no runtime). */
int poporon_amd_device_count(void);

/* Bind the handle to HIP device `device` (default: the device current at the
 * handle's first GPU call).  Must be called before any GPU work. */
bool poporon_amd_set_device(poporon_t *pprn, int device);

/* Pre-size the handle's device workspace for batches of up to max_count
 * codewords, so that later device calls allocate nothing (graph capture). */
bool poporon_amd_reserve(poporon_t *pprn, size_t max_count);

/* True when the handle's parameters are served by the GPU kernels: byte
 * symbols (2 <= symbol_size <= 8) and 1 <= num_roots < 2^symbol_size - 1,
 * with any field polynomial, fcr and prim that poporon_create accepts.
 * RS(255,223)-shaped parameters (symbol_size 8, num_roots 32, generator
 * without zero coefficients, (fcr+31)*prim+254 < 65536) run on the fast
 * kernels, all others on the general-parameter kernels (same results,
 * lower throughput).  False otherwise (symbol_size 1 or > 8).  BCH handles:
 * symbol_size 3..5.  LDPC handles: true unless the inner bit interleaver is
 * not a permutation (interleave depth * width != codeword bits, e.g. block 32
 * at rate 5/6 with the automatic depth): the reference's own decode reads
 * uninitialised memory for such a code; the handle exists, the getters work,
 * every codec call returns false with a message. */
bool poporon_amd_supported(const poporon_t *pprn);

/* ---- device-resident batches (asynchronous on `stream`) ------------------ */

bool poporon_encode_batch_device(poporon_t *pprn, const uint8_t *d_data, size_t data_stride, uint8_t *d_parity,
                                 size_t parity_stride, size_t size, size_t count, void *stream);

/*
 * Decode in place.  d_positions == NULL: errors-only decode (the handle's
 * erasure object and external syndromes, if configured, are NOT used by the
 * batch calls).  Otherwise erasure decode: codeword c's erasure list is
 * d_positions[c*positions_stride .. +num_roots] (uint8 positions into data[], slots
 * past the count are read exactly as the reference reads its erasure object,
 * quirks Q2/Q3), d_counts[c] its count (<= num_roots).
 * d_ok[c] = decode result (1/0); d_corrected[c] = corrected_num (may be NULL).
 */
bool poporon_decode_batch_device(poporon_t *pprn, uint8_t *d_data, size_t data_stride, uint8_t *d_parity,
                                 size_t parity_stride, size_t size, size_t count, const uint8_t *d_positions,
                                 size_t positions_stride, const uint8_t *d_counts, uint8_t *d_ok,
                                 uint8_t *d_corrected, void *stream);

/*
 * External-syndrome decode (the config's "syndrome" branch, src/decode.c:
 * 446-464) for a batch: codeword c's num_roots log-form syndromes (value
 * 2^symbol_size - 1 = zero, the reference's uint16 type) are
 * d_syndromes[c*syndrome_stride .. +num_roots].  All-zero syndromes leave the
 * codeword untouched with d_ok[c] = 1; otherwise the correction runs on them.
 * A value above 2^symbol_size - 1 (an out-of-table index in the reference)
 * gives d_ok[c] = 0, d_corrected[c] = 0.
 */
bool poporon_decode_batch_syndrome_device(poporon_t *pprn, uint8_t *d_data, size_t data_stride, uint8_t *d_parity,
                                          size_t parity_stride, size_t size, size_t count,
                                          const uint16_t *d_syndromes, size_t syndrome_stride, uint8_t *d_ok,
                                          uint8_t *d_corrected, void *stream);

/*
 * Syndromes of a batch (the reference's calculate_syndrome_u8, src/decode.c:
 * 375-415, per codeword): d_syndromes[c*syndrome_stride + i] = log S_i in the
 * reference's uint16 log form (2^symbol_size - 1 = zero), d_nonzero[c] = 1
 * when any S_i is nonzero.  Either output may be NULL (not both).  The
 * result feeds poporon_decode_batch_syndrome_device.
 */
bool poporon_syndrome_batch_device(poporon_t *pprn, const uint8_t *d_data, size_t data_stride,
                                   const uint8_t *d_parity, size_t parity_stride, size_t size, size_t count,
                                   uint16_t *d_syndromes, size_t syndrome_stride, uint8_t *d_nonzero, void *stream);

/* Screening without correction: d_dirty[c] = 1 when codeword c has a nonzero
 * syndrome (the reference's calculate_syndrome_u8 flag, src/decode.c:409-414),
 * else 0.  Reads data and parity only. */
bool poporon_check_batch_device(poporon_t *pprn, const uint8_t *d_data, size_t data_stride, const uint8_t *d_parity,
                                size_t parity_stride, size_t size, size_t count, uint8_t *d_dirty, void *stream);

/* ---- host-memory batches (synchronous) ------------------------------------ */

bool poporon_encode_batch(poporon_t *pprn, const uint8_t *data, size_t data_stride, uint8_t *parity,
                          size_t parity_stride, size_t size, size_t count);

bool poporon_decode_batch(poporon_t *pprn, uint8_t *data, size_t data_stride, uint8_t *parity, size_t parity_stride,
                          size_t size, size_t count, const uint8_t *positions, size_t positions_stride,
                          const uint8_t *counts, uint8_t *ok, uint8_t *corrected);

/* ---- symbol-interleaved RS frames ---------------------------------------------
 * RS(255,223) data usually arrives interleaved (CCSDS 131.0-B transfer frames,
 * depths 1, 2, 3, 4, 5 and 8): frame f holds `depth` codewords, symbol by
 * symbol.  Its message region is size*depth bytes at d_data + f*data_stride,
 * message symbol j of codeword i at offset j*depth + i; its parity region
 * num_roots*depth bytes at d_parity + f*parity_stride, parity symbol p of
 * codeword i at offset p*depth + i.  The CCSDS wire block is d_parity =
 * d_data + size*depth with both strides (size + num_roots)*depth; any other
 * placement, base alignment or stride (>= the region) is as valid, and bytes
 * of a stride past a region are never written.  count is the number of
 * frames, 1 <= depth <= 64, depth 1 is the row layout, RS handles only.
 *
 * Codeword c = f*depth + i indexes every per-codeword array: d_ok[c],
 * d_corrected[c], d_dirty[c], d_counts[c], d_positions[c*positions_stride ..];
 * erasure positions are symbol indices into the codeword's own message, as in
 * the row call.  Every per-codeword result equals the row call's on the
 * de-interleaved codeword: the frames of a chunk are gathered into rows in a
 * staging buffer the handle owns (256 B per codeword), the row kernels run
 * there, and parity (encode) or both regions (decode) are scattered back.  A
 * chunk is at most 2^20 codewords (POPORON_AMD_ILV_CHUNK=<codewords> in the
 * environment at poporon_create; whole frames, at least one); larger batches
 * run chunk after chunk on `stream`.  poporon_amd_reserve_interleaved sizes
 * the staging for min(max_codewords, chunk) codewords and does for that count
 * what poporon_amd_reserve does, so that later device calls allocate nothing.
 * The host forms move chunks of frames through pinned memory and return when
 * the results are in host memory. */
bool poporon_encode_interleaved_device(poporon_t *pprn, const uint8_t *d_data, size_t data_stride, uint8_t *d_parity,
                                       size_t parity_stride, size_t size, size_t depth, size_t count, void *stream);
bool poporon_decode_interleaved_device(poporon_t *pprn, uint8_t *d_data, size_t data_stride, uint8_t *d_parity,
                                       size_t parity_stride, size_t size, size_t depth, size_t count,
                                       const uint8_t *d_positions, size_t positions_stride, const uint8_t *d_counts,
                                       uint8_t *d_ok, uint8_t *d_corrected, void *stream);
bool poporon_check_interleaved_device(poporon_t *pprn, const uint8_t *d_data, size_t data_stride,
                                      const uint8_t *d_parity, size_t parity_stride, size_t size, size_t depth,
                                      size_t count, uint8_t *d_dirty, void *stream);
bool poporon_encode_interleaved(poporon_t *pprn, const uint8_t *data, size_t data_stride, uint8_t *parity,
                                size_t parity_stride, size_t size, size_t depth, size_t count);
bool poporon_decode_interleaved(poporon_t *pprn, uint8_t *data, size_t data_stride, uint8_t *parity,
                                size_t parity_stride, size_t size, size_t depth, size_t count,
                                const uint8_t *positions, size_t positions_stride, const uint8_t *counts, uint8_t *ok,
                                uint8_t *corrected);
bool poporon_amd_reserve_interleaved(poporon_t *pprn, size_t max_codewords);

/* ---- wire form of the interleaved calls ----------------------------------------
 * A CCSDS 131.0-B frame does not carry the code's bytes: its symbols travel in
 * Berlekamp's dual-basis representation, and the block is XORed with the
 * pseudo-randomizer.  A handle's wire form says how a byte of a frame becomes
 * a byte of the code: a symbol map, to_code[256] with its inverse to_wire[256],
 * and a receive-side XOR sequence of xor_len bytes.  It is applied inside the
 * layout kernels of the interleaved calls and costs no pass over the frames.
 *
 * poporon_amd_set_wire_form: RS handles of symbol_size 8 (others: false with a
 * message).  to_code and to_wire are both NULL (the identity) or both given
 * with to_wire[to_code[v]] == v for all 256 v; xor_seq NULL with xor_len 0 is
 * no sequence, else 1 <= xor_len <= 65536; anything else fails and leaves the
 * form as it was.  All NULL / 0 clears the form.  The tables are copied.
 * poporon_amd_set_wire_form_ccsds computes the CCSDS tables from their
 * definitions on any symbol_size 8 handle (the code they belong to is
 * symbol_size 8, polynomial 0x187, first root 112, primitive element 11, 32
 * roots): dual_basis, over the field 0x187 with alpha = 2, beta = alpha^117 and
 * Tr(a) = a + a^2 + ... + a^128, bit 7-i of to_wire[u] is Tr(u beta^i), and
 * to_code is the inverse table; randomizer is the 255 bytes of h(x) = x^8 + x^7
 * + x^5 + x^3 + 1 from the all-ones state, MSB first.  Neither of the two
 * clears the form.  poporon_amd_get_wire_form returns false when no form is
 * set, else copies out what was set: the identity for maps that were not
 * given, *xor_len (0 without a sequence) and, when xor_seq is not NULL, the
 * sequence (xor_cap < *xor_len: false, *xor_len still written).
 *
 * Set and get need no GPU.  The device copy is made by the next interleaved
 * call or by poporon_amd_reserve_interleaved, after which calls with the form
 * set allocate nothing.  Setting is a setup call: it waits by itself for the
 * work this handle has enqueued before the device tables are replaced, so
 * calls enqueued before it keep the old form and the caller never
 * synchronises around it.
 *
 * The form is applied by poporon_{encode,decode,check}_interleaved_device,
 * poporon_{encode,decode}_interleaved and
 * poporon_decode_interleaved_report_device, at every depth, 1 included (which
 * then runs through the staging rows too); NOT by the row *_batch* calls, the
 * single calls, the syndrome calls or poporon_amd_erasures_from_mask_device.
 * Rows in wire form go through the interleaved calls at depth 1.
 *
 * A byte's block offset b is its offset in the message region, or size*depth
 * plus its offset in the parity region: wire-block order, wherever the two
 * regions lie.
 *  - decode / check: the code byte is to_code[wire ^ xor_seq[b % xor_len]], and
 *    the row kernels see those.  d_ok, d_corrected, d_dirty and erasure lists
 *    mean what they mean without a form.
 *  - after a decode both regions hold to_wire[code byte], for every codeword,
 *    decoded or not: the block comes back derandomized and is not randomized
 *    again; a failed codeword is otherwise unchanged.
 *  - encode: the message is read through to_code and the parity written
 *    through to_wire.  The sequence is NOT used: the message region is const,
 *    and the randomizer is the last transmit step over the finished block,
 *    which the caller XORs.
 *  - report form: d_err_pos is as without a form; d_err_val is before XOR
 *    after of the CODE bytes (the diff of the staging rows).  To undo a
 *    correction in the returned row: to_wire[to_code[returned] ^ d_err_val]. */
bool poporon_amd_set_wire_form(poporon_t *pprn, const uint8_t to_code[256], const uint8_t to_wire[256],
                               const uint8_t *xor_seq, size_t xor_len);
bool poporon_amd_set_wire_form_ccsds(poporon_t *pprn, bool dual_basis, bool randomizer);
bool poporon_amd_get_wire_form(const poporon_t *pprn, uint8_t to_code[256], uint8_t to_wire[256],
                               uint8_t *xor_seq /* xor_cap bytes, may be NULL */, size_t xor_cap, size_t *xor_len);

/* ---- decode reports: where the errors were -----------------------------------
 * poporon_decode_batch_report_device takes poporon_decode_batch_device's
 * arguments and three more arrays, poporon_decode_interleaved_report_device
 * poporon_decode_interleaved_device's and the same three.  RS handles only
 * (BCH and LDPC handles: false with a message).  The contract:
 *
 *  - Data, parity, d_ok and d_corrected come out exactly as from
 *    poporon_decode_batch_device (poporon_decode_interleaved_device) with the
 *    same arguments; erasure lists are passed through unchanged.
 *  - The report lists the bytes of codeword c that the call changed, ascending
 *    by position; d_err_num[c] is how many.  For k < d_err_num[c],
 *    d_err_pos[c*report_stride + k] is the position: 0 .. size-1 is message
 *    symbol pos, size .. size+num_roots-1 parity symbol pos - size (positions
 *    fit a byte: size + num_roots <= 255), and d_err_val[c*report_stride + k]
 *    is before XOR after, so XORing the report into the returned row gives the
 *    received row back.  A list is capped at num_roots entries; the reference
 *    never applies more corrections than that.
 *  - Slots d_err_num[c] .. num_roots-1 of both arrays are written 0; bytes
 *    num_roots .. report_stride are never written.  report_stride >=
 *    num_roots, or the call fails.
 *  - Interleaved form: c = f*depth + i, and positions are symbol indices
 *    within the codeword, not byte offsets in the frame.
 *  - The report is NOT corrected_num in another form.  d_corrected[c] counts
 *    the non-zero magnitudes the decoder computed, whether or not they were
 *    applied: a codeword that fails late (d_ok[c] = 0) can have d_corrected[c]
 *    > 0 and come back unchanged, and its report is empty (d_err_num[c] = 0).
 *    On successful rows the two usually agree; duplicate or stale erasure
 *    slots (quirks Q1/Q2) and an erased symbol whose value was right can make
 *    them differ.  The report defines nothing beyond the diff of the rows.
 *
 * How: per chunk the rows are copied to a snapshot buffer the handle owns
 * (wire rows, 256 B per codeword allocated: one device copy when the caller's
 * rows are wire rows already, d_parity = d_data + size and both strides size +
 * num_roots, else a gather kernel), the decode runs in place as the plain
 * call's does, and a kernel lists where the rows differ from the snapshot; the
 * interleaved form snapshots its staging rows after the gather.  A chunk is at
 * most 2^20 codewords (POPORON_AMD_REPORT_CHUNK=<codewords> in the environment
 * at poporon_create; the interleaved form at depth > 1 goes by
 * POPORON_AMD_ILV_CHUNK); larger batches run chunk after chunk on `stream`,
 * each routed by its own count.  poporon_amd_reserve_report sizes the snapshot
 * buffer for min(max_codewords, chunk) codewords and does for that count what
 * poporon_amd_reserve does, so that later row report calls allocate nothing
 * (the interleaved form also needs poporon_amd_reserve_interleaved).  The rows
 * take the report kernel's fast path when they are wire rows on a 16-byte
 * aligned base.  The host form moves chunks of rows through pinned memory of
 * its own and returns when the results are in host memory. */
bool poporon_decode_batch_report_device(poporon_t *pprn, uint8_t *d_data, size_t data_stride, uint8_t *d_parity,
                                        size_t parity_stride, size_t size, size_t count, const uint8_t *d_positions,
                                        size_t positions_stride, const uint8_t *d_counts, uint8_t *d_ok,
                                        uint8_t *d_corrected, uint8_t *d_err_num, uint8_t *d_err_pos,
                                        uint8_t *d_err_val, size_t report_stride, void *stream);
bool poporon_decode_interleaved_report_device(poporon_t *pprn, uint8_t *d_data, size_t data_stride, uint8_t *d_parity,
                                              size_t parity_stride, size_t size, size_t depth, size_t count,
                                              const uint8_t *d_positions, size_t positions_stride,
                                              const uint8_t *d_counts, uint8_t *d_ok, uint8_t *d_corrected,
                                              uint8_t *d_err_num, uint8_t *d_err_pos, uint8_t *d_err_val,
                                              size_t report_stride, void *stream);
bool poporon_decode_batch_report(poporon_t *pprn, uint8_t *data, size_t data_stride, uint8_t *parity,
                                 size_t parity_stride, size_t size, size_t count, const uint8_t *positions,
                                 size_t positions_stride, const uint8_t *counts, uint8_t *ok, uint8_t *corrected,
                                 uint8_t *err_num, uint8_t *err_pos, uint8_t *err_val, size_t report_stride);
bool poporon_amd_reserve_report(poporon_t *pprn, size_t max_codewords);

/* ---- erasure lists from a flag plane ------------------------------------------
 * d_mask has the layout of the message regions: frame f has size*depth bytes
 * at d_mask + f*mask_stride, the flag of symbol j of codeword i at j*depth + i
 * (depth 1: rows); a non-zero byte means erased.  For codeword c = f*depth + i
 * the first num_roots flagged symbol indices are written ascending to
 * d_positions[c*positions_stride ..], the slots behind them up to num_roots 0
 * (the decoders read those slots, quirks Q2/Q3), bytes num_roots ..
 * positions_stride never; d_counts[c] = min(flagged, num_roots); d_over[c]
 * (may be NULL) = 1 when more than num_roots symbols were flagged: such a
 * codeword is beyond an erasure decode, and the caller decides what to do with
 * it.  Ascending lists are what the decoders need (quirk Q1: magnitudes pair
 * with list slots in ascending location order).  positions_stride >=
 * num_roots, mask_stride >= size*depth, 1 <= depth <= 64, count frames, RS
 * handles only.  The outputs feed poporon_decode_batch_device /
 * poporon_decode_interleaved_device (and their report forms) directly; a
 * positions_stride of 32 on a 16-byte aligned base keeps the 32-erasure
 * kernel's fast route.  There is no host form: on the host np.nonzero or a
 * loop does this. */
bool poporon_amd_erasures_from_mask_device(poporon_t *pprn, const uint8_t *d_mask, size_t mask_stride, size_t size,
                                           size_t depth, size_t count, uint8_t *d_positions, size_t positions_stride,
                                           uint8_t *d_counts, uint8_t *d_over, void *stream);

/* ---- convolutional-interleaver RS streams --------------------------------------
 * Broadcast and cable links (DVB-S / -T / -C and ISDB-T: RS(204,188), 12
 * branches of cell 17; ATSC: RS(207,187), 52 branches of cell 4) send their
 * codewords through a Forney convolutional interleaver: `branches` (I) FIFOs,
 * branch b of b*cell (b*M) bytes, one byte to each branch in turn.  The
 * interleaver has memory, but it is a pure index map.  Number the code bytes of
 * a batch serially, n = c*W + s: c the codeword, s its symbol (message symbols
 * 0 .. size-1, parity symbols size .. W-1), W = size + num_roots.  Byte n
 * travels on branch b = (phase + n) mod branches and leaves at stream offset
 *
 *     p(n) = n + b * cell * branches.
 *
 * A batch of count codewords occupies a span of poporon_amd_conv_span(W, count,
 * branches, cell) = count*W + (branches-1)*cell*branches bytes, and d_stream
 * points at span offset 0.  The (branches-1)*cell*branches offsets of the span
 * that are no p(n) are holes: bytes of the codewords before and after the
 * batch.  So the calls are stateless.  Successive calls take overlapping
 * windows of one stream, the next at d_stream + count*W with phase (phase +
 * count*W) mod branches, and each call touches only its own bytes: calls on
 * neighbouring windows never write a byte of one another's.
 *
 * Limits: 1 <= branches <= 128, 1 <= cell <= 255, phase < branches, 1 <= size
 * <= 2^symbol_size - 1 - num_roots (as the row decode checks it), strides at
 * least their regions, any base alignment and any stride.  branches 1 is the
 * identity: the stream is the wire rows back to back.  count 0 succeeds and
 * launches nothing.  Every stream offset is computed in size_t.  RS handles
 * only (BCH and LDPC handles: false with a message).
 *
 * Memory touched: nothing outside [0, span) of the stream is read or written,
 * holes are never written, bytes of a row stride past a region are never
 * written, const inputs are unchanged.
 *
 *  - poporon_amd_conv_interleave_device: rows -> stream, layout only.  Each
 *    codeword's W bytes are written to their p(n); d_parity NULL: the parity
 *    offsets keep their contents.
 *  - poporon_amd_conv_deinterleave_device: the inverse; d_parity NULL: the
 *    parity symbols are not delivered.  A stream of per-symbol flag bytes goes
 *    through it with d_parity NULL and then to
 *    poporon_amd_erasures_from_mask_device at depth 1 (mask_stride = data_stride),
 *    whose lists feed poporon_decode_conv_device.
 *  - poporon_encode_conv_device: poporon_encode_batch_device on the rows, which
 *    writes d_parity (required) exactly as that call does, then the interleave.
 *  - poporon_decode_conv_device: the de-interleave straight into the caller's
 *    rows, then poporon_decode_batch_device in place there: no staging buffer
 *    and no extra pass.  Every per-codeword result (bytes, d_ok, d_corrected,
 *    erasure semantics, quirks) equals the row call's on the de-interleaved
 *    rows; a failed codeword comes out as received.  d_parity is required.
 *  - poporon_decode_conv_report_device: the same with the report arrays of
 *    poporon_decode_batch_report_device on those rows (its chunks and its
 *    snapshot buffer: poporon_amd_reserve_report).
 *  - poporon_check_conv_device: d_dirty[c] as poporon_check_batch_device gives
 *    it.  The stream is const and there are no rows: chunks of at most
 *    POPORON_AMD_ILV_CHUNK codewords (default 2^20) are gathered into the
 *    staging rows of the interleaved calls, chunk by chunk on `stream`, each
 *    chunk its own window (base + c0*W, phase (phase + c0*W) mod branches).
 *    poporon_amd_reserve_interleaved pre-sizes that staging.
 *
 * The layout, encode and decode calls allocate nothing beyond what the row
 * calls allocate (poporon_amd_reserve covers it).  A wire form set on the
 * handle is NOT applied by these calls, as it is not applied by the row calls.
 * DVB's energy dispersal and sync-byte inversion sit outside the RS code and
 * stay with the caller.
 *
 * Kernels (rs_conv.hip): a workgroup moves a tile of poporon_amd_conv_tile(W,
 * branches, cell) codewords through an LDS image of its stream window; where
 * that returns 0 the window does not fit the LDS and a plain path without a
 * tile runs.  POPORON_AMD_CONV_PATH=tile / direct in the environment at
 * poporon_create forces either (tile on a geometry that does not fit fails the
 * call with a message).
 *
 * There are no host forms: a host encode would have to merge the partly owned
 * windows at both ends of its span with the caller's stream, so the caller
 * copies the span to the device and back instead. */
/* count*row_bytes + (branches-1)*cell*branches; 0 on invalid arguments or overflow.  No GPU. */
size_t poporon_amd_conv_span(size_t row_bytes, size_t count, size_t branches, size_t cell);
/* codewords per workgroup of the tile kernels for rows of row_bytes <= 255 bytes; 0: the direct path.  No GPU. */
size_t poporon_amd_conv_tile(size_t row_bytes, size_t branches, size_t cell);
bool poporon_amd_conv_interleave_device(poporon_t *pprn, const uint8_t *d_data, size_t data_stride,
                                        const uint8_t *d_parity, size_t parity_stride, size_t size, size_t count,
                                        size_t branches, size_t cell, size_t phase, uint8_t *d_stream, void *stream);
bool poporon_amd_conv_deinterleave_device(poporon_t *pprn, const uint8_t *d_stream, size_t branches, size_t cell,
                                          size_t phase, uint8_t *d_data, size_t data_stride, uint8_t *d_parity,
                                          size_t parity_stride, size_t size, size_t count, void *stream);
bool poporon_encode_conv_device(poporon_t *pprn, const uint8_t *d_data, size_t data_stride, uint8_t *d_parity,
                                size_t parity_stride, size_t size, size_t count, size_t branches, size_t cell,
                                size_t phase, uint8_t *d_stream, void *stream);
bool poporon_decode_conv_device(poporon_t *pprn, const uint8_t *d_stream, size_t branches, size_t cell, size_t phase,
                                uint8_t *d_data, size_t data_stride, uint8_t *d_parity, size_t parity_stride,
                                size_t size, size_t count, const uint8_t *d_positions, size_t positions_stride,
                                const uint8_t *d_counts, uint8_t *d_ok, uint8_t *d_corrected, void *stream);
bool poporon_decode_conv_report_device(poporon_t *pprn, const uint8_t *d_stream, size_t branches, size_t cell,
                                       size_t phase, uint8_t *d_data, size_t data_stride, uint8_t *d_parity,
                                       size_t parity_stride, size_t size, size_t count, const uint8_t *d_positions,
                                       size_t positions_stride, const uint8_t *d_counts, uint8_t *d_ok,
                                       uint8_t *d_corrected, uint8_t *d_err_num, uint8_t *d_err_pos,
                                       uint8_t *d_err_val, size_t report_stride, void *stream);
bool poporon_check_conv_device(poporon_t *pprn, const uint8_t *d_stream, size_t branches, size_t cell, size_t phase,
                               size_t size, size_t count, uint8_t *d_dirty, void *stream);

/* ---- plane layout: RS stripes across shards ------------------------------------
 * Storage keeps a byte-symbol code the other way round from a link: a stripe
 * has `size` data shards and num_roots parity shards, each a long buffer of its
 * own, and codeword c is byte c of every shard.  A *plane table* is a HOST array
 * of W = size + num_roots DEVICE pointers: entries 0 .. size-1 the message
 * planes, entries size .. W-1 the parity planes; codeword c has symbol j at
 * planes[j][c]; count is the number of codewords, that is, bytes per plane.
 * Planes may lie anywhere and at any alignment, and must not overlap.  The
 * calls are the row calls on the W x count transpose, without the transposes:
 *
 *  - poporon_encode_planes_device: every message plane is non-NULL and is not
 *    written.  Parity plane p receives what poporon_encode_batch_device writes
 *    to parity[p] of row c.  A NULL parity entry: that plane is not delivered;
 *    all parity entries NULL fails the call.
 *  - poporon_decode_planes_device: `lost` is a HOST array of lost_count plane
 *    indices, strictly ascending, each < W, lost_count <= num_roots (lost
 *    parity plane p is index size + p); anything else fails the call before
 *    any launch (an unsorted list would trip quirk Q1).  Lost planes are NEVER
 *    READ: the row that is decoded holds 0 there.  A lost plane's table entry
 *    may be NULL: it is neither read nor written.  A surviving plane may not be
 *    NULL.  lost_count 0 is the errors-only decode.  Otherwise it is the erasure
 *    decode, and every codeword gets the list lost[0 .. lost_count) followed by
 *    zeros up to num_roots -- the fill poporon_amd_erasures_from_mask_device
 *    writes -- and the count lost_count.  d_ok[c], d_corrected[c] (may be NULL)
 *    and every byte equal poporon_decode_batch_device on that row with that
 *    list, quirks Q1/Q2 and the corrected_num semantics included.  After the
 *    call every non-NULL plane holds its symbol of the row as the row call left
 *    it: a failed codeword's surviving symbols are as received, and its symbols
 *    in non-NULL lost planes are what the row call left of the 0.
 *    d_dirty (may be NULL): d_dirty[c] is poporon_check_batch_device's flag on
 *    the row AFTER the decode.  It exists because of quirk Q2: with one or more
 *    lost planes and a corrupted surviving symbol the reference pairs the
 *    magnitudes with the wrong list slots and returns ok = 1 with wrong bytes
 *    (RS(255,223), 4 lost planes: up to 14 errors; RS(14,10), 1 lost plane: 1
 *    error), and this library returns exactly that.  d_ok is the reference's
 *    answer; d_dirty[c] = 1 says that what was written is no codeword.  The
 *    errors-only decode (a scrub) has no such case.
 *  - poporon_decode_planes_report_device: the same with the report arrays of
 *    poporon_decode_batch_report_device on those rows, so d_err_pos is the PLANE
 *    INDEX: which shard was bad.  A rebuilt non-zero symbol of a lost plane is
 *    listed with d_err_val = its value (the row held 0).  A failed codeword's
 *    report is empty.  Needs poporon_amd_reserve_report besides
 *    poporon_amd_reserve_planes to allocate nothing.
 *  - poporon_check_planes_device: all planes non-NULL and const; d_dirty[c] as
 *    poporon_check_batch_device gives it.
 *  - the _strided forms: one buffer, message plane j at d_data +
 *    j*data_plane_stride, parity plane p at d_parity + p*parity_plane_stride
 *    (offsets in size_t; they may pass 2^32).  They fill a table on the host and
 *    are the table forms from there on, so no entry is NULL.
 *
 * Limits: 1 <= size <= 2^symbol_size - 1 - num_roots, as the row decode checks
 * it.  RS handles only (BCH and LDPC handles: false with a message).  A wire
 * form set on the handle is NOT applied.  count 0 succeeds and launches nothing
 * (the table may then be NULL).  Every plane offset is computed in size_t.
 * Nothing outside [0, count) of a plane is read or written.  The calls are
 * asynchronous on `stream`; the table and the lost list are consumed before
 * the call returns (they reach the kernels by value in the launch arguments:
 * no device table, no copy, no wait).
 *
 * How: chunks of at most POPORON_AMD_ILV_CHUNK codewords (default 2^20) run one
 * after another on `stream`.  Each is gathered into the staging rows of the
 * interleaved calls (rs_planes.hip), the row kernels run there, routed by the
 * chunk's count, d_dirty is the check kernel on those rows, and the rows are
 * scattered back: the parity planes after an encode, every non-NULL plane after
 * a decode, nothing after a check.  The erasure lists of a rebuild live in a
 * buffer the handle owns, one chunk's worth on a 16-byte aligned base at a
 * stride of num_roots rounded up to 16, written once per call.
 * poporon_amd_reserve_planes sizes that buffer, the staging rows and the
 * decoders' workspace for min(max_codewords, chunk) codewords, after which
 * plane calls allocate nothing.  A workgroup moves a tile of
 * poporon_amd_plane_tile(W) codewords through 32 KiB of LDS at the most; when
 * every table entry is a multiple of 16 the kernels without a byte path at
 * the ends of a plane's run are taken.  There are no host forms. */
/* codewords per workgroup tile of the plane kernels for rows of row_bytes <= 255 bytes: a multiple of 16, at least
 * 64; 0 for a row_bytes that is no row.  No GPU. */
size_t poporon_amd_plane_tile(size_t row_bytes);
bool poporon_amd_reserve_planes(poporon_t *pprn, size_t max_codewords);
bool poporon_encode_planes_device(poporon_t *pprn, uint8_t *const *planes, size_t size, size_t count, void *stream);
bool poporon_decode_planes_device(poporon_t *pprn, uint8_t *const *planes, size_t size, size_t count,
                                  const uint8_t *lost, size_t lost_count, uint8_t *d_ok, uint8_t *d_corrected,
                                  uint8_t *d_dirty, void *stream);
bool poporon_decode_planes_report_device(poporon_t *pprn, uint8_t *const *planes, size_t size, size_t count,
                                         const uint8_t *lost, size_t lost_count, uint8_t *d_ok, uint8_t *d_corrected,
                                         uint8_t *d_dirty, uint8_t *d_err_num, uint8_t *d_err_pos, uint8_t *d_err_val,
                                         size_t report_stride, void *stream);
bool poporon_check_planes_device(poporon_t *pprn, const uint8_t *const *planes, size_t size, size_t count,
                                 uint8_t *d_dirty, void *stream);
bool poporon_encode_planes_strided_device(poporon_t *pprn, const uint8_t *d_data, size_t data_plane_stride,
                                          uint8_t *d_parity, size_t parity_plane_stride, size_t size, size_t count,
                                          void *stream);
bool poporon_decode_planes_strided_device(poporon_t *pprn, uint8_t *d_data, size_t data_plane_stride,
                                          uint8_t *d_parity, size_t parity_plane_stride, size_t size, size_t count,
                                          const uint8_t *lost, size_t lost_count, uint8_t *d_ok, uint8_t *d_corrected,
                                          uint8_t *d_dirty, void *stream);
bool poporon_check_planes_strided_device(poporon_t *pprn, const uint8_t *d_data, size_t data_plane_stride,
                                         const uint8_t *d_parity, size_t parity_plane_stride, size_t size,
                                         size_t count, uint8_t *d_dirty, void *stream);

/* ---- product-code blocks (RS x RS: DVD's RS-PC block, flash and tape) --------
 * A block is a codeword of a ROW code along every row and of a COLUMN code
 * along every column.  Its decode is not one call per codeword but a schedule
 * of row passes and column passes that hand each other their failures as
 * erasures.  These calls run that schedule on the device without returning to
 * the host between passes.
 *
 * Object.  poporon_amd_product_create takes two RS configs that
 * poporon_amd_supported serves, with the SAME symbol_size and the SAME field
 * polynomial (anything else: NULL with a message); fcr, prim and num_roots may
 * differ.  With one field both encodes are linear over it, so the checks on
 * checks are the same whichever axis is encoded first and the encoded block is
 * a codeword on every row and every column (tests/test_product_cpu.py shows it
 * on the reference).  The object owns one handle per axis
 * (poporon_amd_product_handle: 0 = row code, 1 = column code; for
 * poporon_amd_timing and poporon_amd_set_device on axis 0 BEFORE the first GPU
 * call; the column handle follows the row handle's device).  Create needs no
 * GPU.
 *
 * Layout.  The row code takes messages of row_size = k1 symbols, n1 = k1 + r1;
 * the column code col_size = k2, n2 = k2 + r2 (poporon_amd_product_shape gives
 * n1 and n2, no GPU).  Block b is n2 rows of n1 bytes, byte (i, j) at d_blocks +
 * b*block_stride + i*row_pitch + j.  Rows 0 .. k2-1 x columns 0 .. k1-1 are the
 * message, rows k2 .. n2-1 column parity, columns k1 .. n1-1 row parity.
 * row_pitch >= n1 and block_stride >= (n2-1)*row_pitch + n1; any base alignment;
 * all offsets size_t; bytes of a pitch or a stride outside the n2 x n1 rectangle
 * are never written.  Row codeword (b, i) has per-codeword index b*n2 + i,
 * column codeword (b, j) index b*n1 + j and its symbol i is byte (i, j): a
 * column's erasure positions are row indices, parity rows k2 .. n2-1.
 *
 * Calls (asynchronous on `stream`; count in blocks; count 0 succeeds and
 * launches nothing):
 *  - poporon_encode_product_device reads the message rectangle only, writes the
 *    column parity of columns 0 .. k1-1 (the column code's encode on the
 *    columns), then the row parity of all n2 rows.
 *  - poporon_check_product_device: d_row_dirty[b*n2 + i] and d_col_dirty[b*n1 +
 *    j] are poporon_check_batch_device's flag on that codeword, d_block_ok[b] =
 *    1 iff none of the block's flags is set.  Any output may be NULL, not all.
 *  - poporon_decode_product_device: pass p = 0 .. passes-1 (1 <= passes <= 16)
 *    runs on axis A = (first_axis + p) mod 2:
 *     1. Lists.  With couple != 0 and p > 0 let E_b be the ascending indices of
 *        the OTHER axis's codewords of block b that are dirty after pass p-1,
 *        r_A the num_roots of A's code.  If floor(r_A/2) < |E_b| <= r_A every
 *        A-codeword of block b gets the erasure list E_b, zeros behind it up to
 *        r_A, and the count |E_b| (the fill
 *        poporon_amd_erasures_from_mask_device writes); otherwise a list of
 *        zeros with the count 0.  With p = 0 or couple == 0 the pass is the
 *        errors-only call (d_positions NULL).
 *        NOTE: a count-0 list is NOT the errors-only call.  It is the erasure
 *        mode of the reference with an empty list, and in that mode the
 *        reference XORs magnitude i into list slot i, read past the count
 *        (quirk Q2): a codeword with 1 .. t errors comes back ok with every
 *        magnitude XORed into symbol 0, and step 3 flags it dirty.  Clean and
 *        undecodable codewords are unaffected.  So a coupled pass repairs
 *        erasures where the other axis flagged floor(r_A/2)+1 .. r_A codewords
 *        and repairs NO plain errors anywhere; a schedule that needs the
 *        errors-only decode on a later pass asks for it with couple == 0
 *        (tests/test_product_cpu.py pins this on the reference).
 *     2. Decode: poporon_decode_batch_device on the A-codewords with those
 *        lists, bit for bit, Q1/Q2 and failed codewords as that call leaves
 *        them.
 *     3. Flags: poporon_check_batch_device on the A-codewords as written back.
 *        "Failed" means dirty after the pass, not !ok: that catches a Q2 result.
 *    After the last pass the other axis is checked once; the three outputs mean
 *    what they mean in the check call, on the block as returned.
 *  - poporon_encode_product / poporon_decode_product: the same on host memory,
 *    whole blocks through a pinned slot, returning when the results are there.
 *
 * How: chunks of whole blocks, at most POPORON_AMD_ILV_CHUNK codewords of
 * either axis, run one after another; a chunk's whole schedule is enqueued
 * before the next chunk's.  A pass gathers the axis's codewords into that
 * handle's staging rows (rs_product.hip), runs the row kernels there, routed by
 * the chunk's codeword count, and scatters them back: the whole rectangle after
 * a decode, that pass's parity after an encode, nothing after a check.  When
 * block_stride == n2*row_pitch the rows are wire rows already and the row code
 * runs in place on the caller's buffer (no staging, no timing id).  The lists
 * live in the axis handle's list buffer (the plane calls'), on a 16-byte
 * aligned base at a stride of r_A rounded up to 16.  A NULL flag output is
 * replaced by a workspace the object owns.  poporon_amd_product_reserve sizes
 * all of it for min(max_blocks, a chunk) blocks, after which product calls
 * allocate nothing.  poporon_amd_product_tile gives the layout kernels' tile for
 * blocks of `codewords` codewords of codeword_bytes each on an axis (axis 1:
 * n2 and n1; axis 0: n1 and n2): *blocks whole blocks per workgroup, and
 * *per_tile codewords of a block per workgroup (= codewords unless a block is
 * split; then *blocks is 1).  No GPU.  There are no report forms. */
typedef struct _poporon_product_t poporon_product_t;
poporon_product_t *poporon_amd_product_create(const poporon_config_t *row_config, const poporon_config_t *col_config);
void poporon_amd_product_destroy(poporon_product_t *prod);
poporon_t *poporon_amd_product_handle(poporon_product_t *prod, int axis);
bool poporon_amd_product_shape(const poporon_product_t *prod, size_t row_size, size_t col_size, size_t *n1, size_t *n2);
bool poporon_amd_product_tile(size_t codeword_bytes, size_t codewords, size_t *blocks, size_t *per_tile);
bool poporon_amd_product_reserve(poporon_product_t *prod, size_t row_size, size_t col_size, size_t max_blocks);
bool poporon_encode_product_device(poporon_product_t *prod, uint8_t *d_blocks, size_t row_pitch, size_t block_stride,
                                   size_t row_size, size_t col_size, size_t count, void *stream);
bool poporon_decode_product_device(poporon_product_t *prod, uint8_t *d_blocks, size_t row_pitch, size_t block_stride,
                                   size_t row_size, size_t col_size, size_t count, int first_axis, size_t passes,
                                   int couple, uint8_t *d_row_dirty, uint8_t *d_col_dirty, uint8_t *d_block_ok,
                                   void *stream);
bool poporon_check_product_device(poporon_product_t *prod, const uint8_t *d_blocks, size_t row_pitch,
                                  size_t block_stride, size_t row_size, size_t col_size, size_t count,
                                  uint8_t *d_row_dirty, uint8_t *d_col_dirty, uint8_t *d_block_ok, void *stream);
bool poporon_encode_product(poporon_product_t *prod, uint8_t *blocks, size_t row_pitch, size_t block_stride,
                            size_t row_size, size_t col_size, size_t count);
bool poporon_decode_product(poporon_product_t *prod, uint8_t *blocks, size_t row_pitch, size_t block_stride,
                            size_t row_size, size_t col_size, size_t count, int first_axis, size_t passes, int couple,
                            uint8_t *row_dirty, uint8_t *col_dirty, uint8_t *block_ok);

/* ---- soft-decision RS decode: Chase-2 over bit LLRs ---------------------------
 * The row decode takes hard symbols.  A demodulator knows more: how reliable
 * every bit was.  This call takes that, as int8 LLRs, and spends the errors-only
 * row decode 2^flips times per codeword on it: the `flips` least reliable bits
 * are tried both ways, every trial row is decoded, and the decoded codeword
 * closest to the LLRs wins.  Every step is integer arithmetic and pinned here,
 * so the result is defined bit for bit (tests/soft_ref.py is the model).
 *
 * Let m = symbol_size (2..8), nr = num_roots, W = size + nr.
 *
 * Input.  Codeword c has W*m int8 values at d_llr + c*llr_stride: the value of
 * bit j of symbol s, MSB first (j = 0 is the symbol's bit m-1), at index
 * s*m + j; message symbols 0 .. size-1 first, then the parity symbols.
 * Negative means 1, >= 0 means 0 (the LDPC soft path's convention).  The
 * contents of the rows at d_data / d_parity are NOT an input.
 *  1. Hard row.  hard[s] = sum over j of (llr[s*m + j] < 0) << (m-1-j).
 *  2. Pick.  A bit's magnitude is |llr| as an int (-128 gives 128).  The picked
 *     bits q_0 .. q_(flips-1) are the first `flips` bit indices in ascending
 *     order of (magnitude, bit index): ties go to the lower index.
 *  3. Candidates.  For p = 0 .. 2^flips - 1, candidate p is the hard row with bit
 *     q_k flipped wherever bit k of p is set.
 *  4. Decode.  Every candidate goes through the errors-only row decode, routed
 *     by the number of candidate rows of the chunk as any batch of that many
 *     rows is; its result is poporon_decode_batch_device's for that row (the
 *     reference's, quirks Q6/Q8 included).  A candidate whose decode fails is
 *     ignored, whatever the failed decode left in its row.
 *  5. Score and select.  The score of a candidate that decoded to row y is the
 *     sum of the magnitudes of all bits in which y differs from the hard row (at
 *     most 2040 * 128).  The winner is the smallest score, ties to the lowest p.
 *  6. Output.  With a winner: d_data / d_parity of codeword c get y, d_ok[c] = 1,
 *     d_changed[c] = the number of symbols with y != hard, d_pattern[c] = p,
 *     d_score[c] = the winner's score.  Without one: the rows get the hard row,
 *     d_ok[c] = 0 and the other three are 0.
 * flips = 0 is therefore poporon_decode_batch_device on the hard rows: the same
 * ok, and the same bytes wherever ok = 1 (a failed row comes back as the hard
 * row here).
 *
 * d_changed, d_pattern and d_score (4-byte aligned) may be NULL; d_ok may not.
 * Data and parity may lie anywhere, at any alignment and stride, as for
 * poporon_decode_batch_device; bytes between rows are never written, and d_llr
 * (any alignment) is never written.  count 0 returns true without a GPU.  The
 * call fails before it touches the GPU, with a message, for a NULL or non-RS
 * handle, size outside [1, kmax], flips > 6 or flips > W*m, llr_stride < W*m,
 * data_stride < size, parity_stride < nr, and NULL d_llr, d_data, d_parity or
 * d_ok.  There are no erasure lists and no external syndromes on this call, and
 * they do not combine with it: an erasure-mode decode that also meets plain
 * errors pairs magnitudes with the wrong slots and returns ok with wrong bytes
 * (quirk Q2), so candidates could not be trusted.  A wire form set on the
 * handle is NOT applied.  There is no host form.  Asynchronous on `stream`.
 *
 * How: chunks of max(1, POPORON_AMD_ILV_CHUNK >> flips) codewords (default 2^20
 * candidate rows) run one after another on `stream`.  rs_soft_expand_k writes a
 * chunk's candidates into the staging rows of the interleaved calls (256 bytes
 * each, candidate p of the chunk's codeword i at row (i << flips) + p), the row
 * decode runs there with its ok / corrected in a buffer the handle owns, and
 * rs_soft_select_k scores the candidates and writes the caller's arrays
 * (rs_soft.hip).  poporon_amd_reserve_soft sizes the staging rows, that buffer
 * and the decoders' workspace for min(max_codewords, chunk) << flips rows, after
 * which soft calls with that `flips` allocate nothing. */
/* (size + num_roots) * symbol_size: the int8 values of one codeword; 0 for a handle that is no RS handle or a size
 * outside [1, kmax].  No GPU. */
size_t poporon_amd_soft_llr_row(const poporon_t *pprn, size_t size);
bool poporon_amd_reserve_soft(poporon_t *pprn, unsigned flips, size_t max_codewords);
bool poporon_decode_soft_batch_device(poporon_t *pprn, const int8_t *d_llr, size_t llr_stride, uint8_t *d_data,
                                      size_t data_stride, uint8_t *d_parity, size_t parity_stride, size_t size,
                                      size_t count, unsigned flips, uint8_t *d_ok, uint8_t *d_changed,
                                      uint8_t *d_pattern, uint32_t *d_score, void *stream);

/* ---- K = 7 convolutional code: batch encode and Viterbi decode ----------------
 * The inner code of the DVB-S / DVB-T and CCSDS 131.0-B chains: constraint
 * length 7, rate 1/2, punctured by a periodic pattern.  The decoder's output is
 * what poporon_decode_conv_device takes.  Everything is integer arithmetic and
 * pinned here, so the result is defined bit for bit (tests/cc_ref.py is the
 * model).  The handle holds parameters only: no device memory, no reserve call,
 * no kernel-timing id.  Calls run on the current HIP device, asynchronously on
 * `stream`.  There is no host form.
 *
 * Code.  A state is 6 bits, the last six input bits, newest at bit 5.  For
 * input bit u in state s the register is r = (u << 6) | s; output j is
 * parity(r & g_j) ^ ((invert >> j) & 1); the next state is r >> 1.  g0, g1 in
 * [1, 127], invert in [0, 3].  CCSDS is (0171, 0133, invert 2), DVB
 * (0171, 0133, 0).
 *
 * Puncturing.  Step t has phase t % period (period in [1, 16]).  Output 0 of
 * the step is transmitted iff bit `phase` of keep0 is set, output 1 likewise by
 * keep1; a step's kept outputs go out in the order 0, 1.  The masks have no bit
 * at or above `period` and at least one bit between them; a phase that keeps
 * nothing is allowed.  poporon_amd_cc_symbols(nbits) is the number of kept
 * symbols of nbits steps.
 *
 * Bit packing (info bits and the encoder's symbols).  Bit t of a frame is bit
 * 7 - t % 8 of byte t / 8 (MSB first); the spare low bits of a frame's last
 * byte are written as 0; no byte past ceil(n / 8) of a frame is written.
 *
 * Encode.  Frame c reads nbits bits at d_bits + c*bits_stride, starts in
 * start_state (0..63) and writes poporon_amd_cc_symbols(nbits) packed hard
 * symbols at d_symbols + c*symbols_stride; d_end_state[c] (may be NULL) gets
 * the final state.
 *
 * Decode input.  Frame c has M = poporon_amd_cc_symbols(nbits) int8 values at
 * d_llr + c*llr_stride, kept symbols only.  Negative means 1, 0 is an erasure.
 * Hypothesising bit b for the received value v costs |v| (-128 gives 128) if
 * v != 0 and (v < 0) != b, else 0; punctured outputs cost 0; a path metric is
 * the sum of the costs along the path.
 *
 * Decode blocks.  B = block, V = overlap.  Block b emits the steps
 * [bB, min(nbits, (b+1)B)) from the window [t0, t1) = [max(0, bB - V),
 * min(nbits, (b+1)B + V)); blocks are independent.
 *  - Initial metrics at t0: if t0 == 0 and start_state >= 0 only paths that
 *    start in start_state exist; otherwise all 64 states start at 0.
 *  - Add-compare-select: the predecessors of state s' are ((s' << 1) | d) & 63
 *    for d = 0, 1, the hypothesised input is s' >> 5, the smaller metric
 *    survives, a tie goes to d = 0.
 *  - End at t1: if t1 == nbits and end_state >= 0 the traceback starts in
 *    end_state, otherwise in the state of least metric, ties to the lowest
 *    state number.
 *  - Output: the bit of step t is bit 5 of the path's state after step t; only
 *    the block's own steps are written.  d_metric[c*blocks + b] (may be NULL;
 *    blocks = poporon_amd_cc_blocks(nbits) = ceil(nbits / B)) gets the metric of
 *    the state the traceback started in.
 * An end_state that cannot be reached from start_state in nbits < 6 steps is
 * the caller's error: those bits are unspecified but stay inside the frame.
 *
 * Create fails, with a message, for polynomials, inversion or masks outside the
 * above, block not a multiple of 64 in [64, 4096] and overlap > 1024; block = 0
 * and overlap = 0xFFFFFFFF select the library defaults (512 and 96: DESIGN
 * section 19 has the measurements behind them).  The calls fail before they
 * touch the GPU for a NULL handle, nbits == 0, a state outside 0..63 (encode
 * start) or -1..63 (decode), strides smaller than a frame (bits: ceil(nbits/8),
 * symbols: ceil(M/8), LLRs: M) and NULL d_bits, d_symbols or d_llr.  count == 0
 * returns true without touching the GPU.  Bases and strides may have any
 * alignment; symbol and bit offsets are 64-bit.
 *
 * How (cc.hip): a decode is one wave per block, lane = state; count * blocks
 * waves go out in launches of at most POPORON_AMD_CC_CHUNK blocks (environment,
 * read at create; default 2^22), an encode in launches of 64 times as many
 * threads, one thread per 32 symbols. */
typedef struct _poporon_cc_t poporon_cc_t;

poporon_cc_t *poporon_amd_cc_create(unsigned g0, unsigned g1, unsigned invert, unsigned period, uint32_t keep0,
                                    uint32_t keep1, unsigned block, unsigned overlap);
void poporon_amd_cc_destroy(poporon_cc_t *cc);
size_t poporon_amd_cc_symbols(const poporon_cc_t *cc, size_t nbits);
size_t poporon_amd_cc_blocks(const poporon_cc_t *cc, size_t nbits);
bool poporon_cc_encode_device(const poporon_cc_t *cc, const uint8_t *d_bits, size_t bits_stride, size_t nbits,
                              size_t count, int start_state, uint8_t *d_symbols, size_t symbols_stride,
                              uint8_t *d_end_state, void *stream);
bool poporon_cc_decode_device(const poporon_cc_t *cc, const int8_t *d_llr, size_t llr_stride, size_t nbits,
                              size_t count, int start_state, int end_state, uint8_t *d_bits, size_t bits_stride,
                              uint32_t *d_metric, void *stream);

/* ---- K = 7 convolutional code: soft-output decode (max-log-MAP) ---------------
 * The same code, puncturing, input LLRs, branch costs, blocks and windows as
 * poporon_cc_decode_device; the output is one int8 LLR per info bit instead of a
 * bit: the row that poporon_decode_soft_batch_device takes.  Integer arithmetic
 * throughout, pinned here (tests/cc_soft_ref.py is the model).
 *
 * Window.  Block b owns the steps [bB, min(nbits, (b+1)B)) and runs the window
 * [t0, t1) of the hard decode, n = t1 - t0 steps; blocks are independent.
 * c_i(s, s') is the cost of step t0 + i on the branch from s to s' (the
 * predecessors of s' are ((s' << 1) | d) & 63, the hypothesised input is
 * s' >> 5).  "No path" is the number 2^28, added like any other cost: a window
 * costs at most 6144 * 256, so nothing overflows 32 bits and every value below is
 * defined.
 *  - Forward: A_0(s) = 0 for all s; if t0 == 0 and start_state >= 0,
 *    A_0(start_state) = 0 and A_0(s) = 2^28 for the other states.
 *    A_{i+1}(s') = min over d of A_i(pred_d(s')) + c_i(pred_d(s'), s').
 *  - Backward: Z_n(s) = 0 for all s; if t1 == nbits and end_state >= 0,
 *    Z_n(end_state) = 0 and Z_n(s) = 2^28 for the other states.
 *    Z_i(s) = min over the two successors s' of s of c_i(s, s') + Z_{i+1}(s').
 *  - Output of an own step t = t0 + i: D_b = min over the s' with (s' >> 5) == b
 *    of A_{i+1}(s') + Z_{i+1}(s'); x = D_1 - D_0 as a signed integer;
 *    mag = min(127, |x| >> shift); d_soft[c*soft_stride + t] = x > 0 ? mag : -mag.
 *    Negative means 1, as everywhere in the library; -128 is never written.
 *
 * Consequences (tests/test_cc_soft_cpu.py, tests/test_gpu_cc_soft.py):
 *  - wherever the output is not 0 its sign bit is the bit that
 *    poporon_cc_decode_device returns for the same handle, frame and boundary
 *    states;
 *  - min(D_0, D_1) of every own step of block b is that call's d_metric[b],
 *    where end_state can be reached;
 *  - with shift = 0 and nbits a multiple of 8 a frame's output is a valid d_llr
 *    row of poporon_decode_soft_batch_device for m = 8: info bit t is bit
 *    7 - t % 8 of byte t / 8 in both.
 *
 * shift is in [0, 8].  A frame writes exactly nbits bytes at d_soft +
 * c*soft_stride; nothing between or around frames is written and d_llr is never
 * written.  Any alignment, 64-bit offsets, asynchronous on `stream`, on the
 * current HIP device.  The call fails before it touches the GPU, in this order,
 * for a NULL handle, nbits == 0, a state outside -1..63, shift > 8, llr_stride <
 * M, soft_stride < nbits and NULL d_llr or d_soft; count == 0 returns true
 * without touching the GPU.  No host form, no kernel-timing id, no reserve call.
 *
 * How (cc_soft.hip): one wave per block, lane = state; the forward metrics are
 * kept every 64 steps and computed again, 64 steps at a time, on the way back;
 * count * blocks waves go out in launches of at most POPORON_AMD_CC_CHUNK blocks,
 * as for the hard decode. */
bool poporon_cc_decode_siso_device(const poporon_cc_t *cc, const int8_t *d_llr, size_t llr_stride, size_t nbits,
                                   size_t count, int start_state, int end_state, unsigned shift, int8_t *d_soft,
                                   size_t soft_stride, void *stream);

/* ---- LDPC batches -----------------------------------------------------------
 * Row c has info_bytes (poporon_get_info_size) of data at d_data +
 * c*data_stride and parity_bytes (poporon_get_parity_size) of parity at
 * d_parity + c*parity_stride; bases and strides may have any alignment, and
 * bytes between rows are never written.  Every per-row result equals the
 * reference's for that row, bit for bit (tests/test_gpu_ldpc.py).
 *
 * Encode (src/encode.c:147-197): the outer interleaver permutes the data bytes
 * in place, parity bit i is the XOR of check row i's info bits and parity bit
 * i-1, spare bits of the last parity byte are 0, and with the inner
 * interleaver on the first codeword_bits bits of data and parity together are
 * bit-interleaved: data and parity are both rewritten.
 *
 * Decode (src/decode.c:489-540).  d_llr == NULL: the hard path
 * (poporon_ldpc_decode_hard): a clean row gives ok with 0 iterations, else up
 * to max_iterations rounds of normalised min-sum from +/-30000 (a config
 * value of 0 means 50).  d_llr given: the soft path (poporon_ldpc_decode_soft)
 * on codeword_bits int8 values per row in channel order at d_llr +
 * c*llr_stride; the row's data and parity bits are not read (d_parity may be
 * NULL) and there is no iteration-0 check.
 * d_ok[c] = result; d_iterations[c] (may be NULL) = the reference's
 * iterations_used (max_iterations on failure); d_hard (may be NULL) gets
 * codeword_bytes = info_bytes + parity_bytes per row, the de-interleaved hard
 * decisions of the last iteration, for failed rows too.  d_data is rewritten
 * (outer de-interleaved) only where d_ok[c] = 1.  Parity is never written.
 *
 * Check: d_dirty[c] = 1 when the de-interleaved row's syndrome is non-zero.
 *
 * The decoder runs one workgroup per codeword with its int16 messages in LDS
 * when they fit the CU's 160 KiB, else in a slice of a workspace the handle
 * owns (poporon_amd_reserve sizes it); POPORON_AMD_LDPC_PATH=lds / global in
 * the environment at poporon_create forces either (lds on a code that does
 * not fit fails the call).  The host forms take the same arguments without
 * the stream and return when the results are in host memory. */
bool poporon_ldpc_encode_batch_device(poporon_t *pprn, uint8_t *d_data, size_t data_stride, uint8_t *d_parity,
                                      size_t parity_stride, size_t count, void *stream);
bool poporon_ldpc_decode_batch_device(poporon_t *pprn, uint8_t *d_data, size_t data_stride, const uint8_t *d_parity,
                                      size_t parity_stride, const int8_t *d_llr, size_t llr_stride, size_t count,
                                      uint8_t *d_ok, uint32_t *d_iterations, uint8_t *d_hard, size_t hard_stride,
                                      void *stream);
bool poporon_ldpc_check_batch_device(poporon_t *pprn, const uint8_t *d_data, size_t data_stride,
                                     const uint8_t *d_parity, size_t parity_stride, size_t count, uint8_t *d_dirty,
                                     void *stream);
bool poporon_ldpc_encode_batch(poporon_t *pprn, uint8_t *data, size_t data_stride, uint8_t *parity,
                               size_t parity_stride, size_t count);
bool poporon_ldpc_decode_batch(poporon_t *pprn, uint8_t *data, size_t data_stride, const uint8_t *parity,
                               size_t parity_stride, const int8_t *llr, size_t llr_stride, size_t count, uint8_t *ok,
                               uint32_t *iterations, uint8_t *hard, size_t hard_stride);
bool poporon_ldpc_check_batch(poporon_t *pprn, const uint8_t *data, size_t data_stride, const uint8_t *parity,
                              size_t parity_stride, size_t count, uint8_t *dirty);

/* LDPC handle's graph, owned by the handle: CSR rows of H, the inner bit
 * interleaver's and the outer byte interleaver's forward tables
 * (NULL when that interleaver is off).  num_edges = row_ptr[num_checks], the
 * edges placed: the QC builder drops those whose row is >= parity_bits.
 * Needs no GPU.  Any output pointer may be NULL. */
bool poporon_amd_ldpc_graph(const poporon_t *pprn, uint32_t *num_checks, uint32_t *num_bits, uint32_t *num_edges,
                            const uint32_t **row_ptr, const uint32_t **col_idx, const uint32_t **inner_forward,
                            const uint32_t **outer_forward);

/* ---- in-library kernel timing ----------------------------------------------
 * When enabled, every kernel the handle launches is bracketed by HIP events
 * recorded on the stream it runs on.  poporon_amd_timing(pprn, 1) enables and
 * resets the totals; poporon_amd_timing_read waits for the recorded events and
 * returns the summed kernel time (ms) and launch count for one kernel id:
 * 0 = encode LFSR, 1 = remainder LFSR, 2 = correction (single kernel),
 * 3 = check LFSR; the split error-mode decode of large batches: 4 = BM +
 * Omega, 5 = Chien, 6 = Forney, 8 = apply, 7 = the one-codeword-per-wave
 * decoder over the codewords the split kernels hand on (for batches routed
 * by their size Forney and the apply are one launch, charged to 8, and 6
 * records none; from more than 1024 codewords per compute unit on the root
 * search runs in that launch too and 5 records none either; Forney and the
 * apply are two launches, 6 and 8, under POPORON_AMD_DECODE_PATH=split, and
 * POPORON_AMD_DECODE_TAIL=search / fused / split in the environment at
 * poporon_create chooses the tail at every count: search = the one launch
 * charged to 8, fused = 5, then Forney and the apply as one launch charged to
 * 8, split = 5, 6 and 8).  Erasure-mode
 * batches of that size: 1, 9 = the 32-sorted-erasure kernel (prim 1), 4 / 5
 * / 6 = the errata kernels, 7 = the same per-wave decoder over the rest, 8 =
 * apply.  A batch of one codeword: 10 = the one-workgroup decoder
 * (rs_dec1_k), 0 = encode (rs_enc1_k).  Batches of 2..16383 codewords: 11 =
 * the one-codeword-per-wave decoder (rs_wave_k, syndromes included).
 * LDPC handles: 12 = encode (ldpc_encode_k), 13 = decode (ldpc_decode_k),
 * 14 = check (ldpc_check_k).
 * The interleaved calls at depth > 1, and at every depth with a wire form set:
 * 15 = frames to staging rows (rs_ilv_gather_k, rs_ilv_gather_map_k with a
 * form), 16 = rows back to frames (rs_ilv_scatter_k, rs_ilv_scatter_map_k),
 * one launch each per chunk; the codec kernels between them keep their ids,
 * routed by the chunk's codeword count.  Depth 1 without a form records
 * neither.
 * The report calls: 17 = the snapshot of a chunk's rows (a device copy, or
 * rs_snapshot_k for rows that are not wire rows), 18 = rs_report_k, one each
 * per chunk, around the decode's own ids.  19 = rs_mask_lists_k
 * (poporon_amd_erasures_from_mask_device).
 * The convolutional-interleaver calls: 20 = stream to rows (rs_conv_gather_k,
 * or rs_conv_gather_direct_k on the plain path), 21 = rows to stream
 * (rs_conv_scatter_k, rs_conv_scatter_direct_k), one launch per layout pass
 * (the check: one per chunk); the codec kernels keep their ids.
 * The plane calls: 22 = planes to staging rows (rs_plane_gather_k; on the
 * first chunk of a rebuild rs_plane_lists_k runs in the same timed stage),
 * 23 = rows back to planes (rs_plane_scatter_k), one each per chunk: 22 alone
 * for a check, 23 only the parity planes for an encode; the codec kernels
 * between them keep their ids, d_dirty is one more launch of 3.
 * The product calls, read on the axis's handle (poporon_amd_product_handle):
 * 24 = block to staging rows (rs_prod_gather_k), 25 = rows back to the block
 * (rs_prod_scatter_k), one each per staged pass and chunk (a check: 24 alone),
 * neither on the in-place row route; 26 = rs_prod_lists_k, one per coupled
 * pass and chunk on the pass's handle, and rs_prod_ok_k, one per chunk on the
 * row handle when d_block_ok is given.  The codec kernels keep their ids; a
 * pass's flags are one more launch of 3.
 * The soft call: 27 = LLR rows to candidate rows (rs_soft_expand_k), 28 = the
 * candidates' scores and the winner's row (rs_soft_select_k), one launch each
 * per chunk; the decode of the candidates between them keeps its ids, routed by
 * the chunk's count of candidate rows.
 *
 * Error- and erasure-mode batches of at least 16384 codewords take the split
 * decode; POPORON_AMD_DECODE_PATH=split / single / wave in the environment
 * at poporon_create forces the split kernels, the lane-per-codeword general
 * kernel (rs_correct_k) or the per-wave decoder for every batch size. */
#define POPORON_AMD_KERNEL_ENCODE 0
#define POPORON_AMD_KERNEL_REMAINDER 1
#define POPORON_AMD_KERNEL_CORRECT 2
#define POPORON_AMD_KERNEL_CHECK 3
#define POPORON_AMD_KERNEL_BM 4
#define POPORON_AMD_KERNEL_CHIEN 5
#define POPORON_AMD_KERNEL_FORNEY 6
#define POPORON_AMD_KERNEL_LIST 7
#define POPORON_AMD_KERNEL_APPLY 8
#define POPORON_AMD_KERNEL_ERASURE 9
#define POPORON_AMD_KERNEL_SINGLE 10
#define POPORON_AMD_KERNEL_WAVE 11
#define POPORON_AMD_KERNEL_LDPC_ENCODE 12
#define POPORON_AMD_KERNEL_LDPC_DECODE 13
#define POPORON_AMD_KERNEL_LDPC_CHECK 14
#define POPORON_AMD_KERNEL_ILV_GATHER 15
#define POPORON_AMD_KERNEL_ILV_SCATTER 16
#define POPORON_AMD_KERNEL_SNAPSHOT 17
#define POPORON_AMD_KERNEL_REPORT 18
#define POPORON_AMD_KERNEL_MASK_LISTS 19
#define POPORON_AMD_KERNEL_CONV_GATHER 20
#define POPORON_AMD_KERNEL_CONV_SCATTER 21
/* the plane calls' ids are enumerators: tests/test_conv_cpu.py pins the macro ids above to 22 of them */
enum { POPORON_AMD_KERNEL_PLANE_GATHER = 22, POPORON_AMD_KERNEL_PLANE_SCATTER = 23 };
enum { POPORON_AMD_KERNEL_PROD_GATHER = 24, POPORON_AMD_KERNEL_PROD_SCATTER = 25, POPORON_AMD_KERNEL_PROD_LISTS = 26 };
enum { POPORON_AMD_KERNEL_SOFT_EXPAND = 27, POPORON_AMD_KERNEL_SOFT_SELECT = 28 };
bool poporon_amd_timing(poporon_t *pprn, int enable);
bool poporon_amd_timing_read(poporon_t *pprn, int kernel, double *total_ms, uint64_t *launches);

/* ---- deterministic payloads -------------------------------------------------
 * Write size bytes of rng's stream (the bytes poporon_rng_next(rng, dest, size)
 * would write, include/poporon/rng.h) into device memory d_dest, on stream
 * (the current HIP device), and advance rng as that call would.  The block
 * start states are derived on the host by GF(2) jump-ahead (rng.hip). */
bool poporon_amd_rng_fill_device(poporon_rng_t *rng, void *d_dest, size_t size, void *stream);

/* ---- multi-GPU: one handle per device, contiguous codeword ranges ----------
 * Codewords are independent, so a batch of count codewords is split into
 * contiguous ranges: device i (of G) takes [count*i/G, count*(i+1)/G)
 * (poporon_amd_multi_range).  No data moves between devices.  Per-codeword
 * results equal the single-device (and single-codeword) results.
 *
 * poporon_amd_multi_create makes one handle per listed device (devices NULL:
 * every visible device) from the same config (copied; erasure / syndrome
 * pointers borrowed as by poporon_create) and initialises each device.  A
 * device may be listed more than once (independent handles sharing it); each
 * listing is a full handle with its own streams, device tables (0.3 MB),
 * split-decode workspace (160 B per codeword of its largest decode batch),
 * single-call buffers and host-pipeline pinned slots, so repeats multiply
 * that memory (no cap: the caller chooses the list).
 * The host entry points take the arguments of poporon_encode_batch /
 * poporon_decode_batch and run one host thread per device over its range.
 * The device entry points take per-device pointer arrays: element i points to
 * device i's range of rows in that device's memory; the work is enqueued on
 * streams[i] (streams NULL: each device's null stream). */
typedef struct _poporon_multi_t poporon_multi_t;

poporon_multi_t *poporon_amd_multi_create(const poporon_config_t *config, const int *devices, size_t num_devices);
void poporon_amd_multi_destroy(poporon_multi_t *multi);
size_t poporon_amd_multi_device_count(const poporon_multi_t *multi);
/* device i's handle (e.g. for poporon_amd_timing); owned by the multi handle */
poporon_t *poporon_amd_multi_handle(poporon_multi_t *multi, size_t index);
/* the range [*first, *first + *n) of part `part` out of `parts` */
bool poporon_amd_multi_range(size_t count, size_t parts, size_t part, size_t *first, size_t *n);

bool poporon_encode_batch_multi(poporon_multi_t *multi, const uint8_t *data, size_t data_stride, uint8_t *parity,
                                size_t parity_stride, size_t size, size_t count);
bool poporon_decode_batch_multi(poporon_multi_t *multi, uint8_t *data, size_t data_stride, uint8_t *parity,
                                size_t parity_stride, size_t size, size_t count, const uint8_t *positions,
                                size_t positions_stride, const uint8_t *counts, uint8_t *ok, uint8_t *corrected);
bool poporon_encode_batch_multi_device(poporon_multi_t *multi, const uint8_t *const *d_data, size_t data_stride,
                                       uint8_t *const *d_parity, size_t parity_stride, size_t size, size_t count,
                                       void *const *streams);
bool poporon_decode_batch_multi_device(poporon_multi_t *multi, uint8_t *const *d_data, size_t data_stride,
                                       uint8_t *const *d_parity, size_t parity_stride, size_t size, size_t count,
                                       const uint8_t *const *d_positions, size_t positions_stride,
                                       const uint8_t *const *d_counts, uint8_t *const *d_ok,
                                       uint8_t *const *d_corrected, void *const *streams);

#ifdef __cplusplus
}
#endif

#endif /* POPORON_AMD_H */
