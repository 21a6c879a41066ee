/*
 * wtp_crc32.h — C-ABI of the MI355X (gfx950) CRC-32 path for WTP.
 *
 * Drop-in boundary for the reference's checksum call surface
 * (mmheyer/a3-reliable-transport):
 *   - inline uint32_t crc32(const void *buf, size_t size)   cpp/src/common/Crc32.hpp:91-102
 *     called from Packet::calculateCheckSum                 cpp/src/base/Packet.cpp:36-38
 *                                                           cpp/src/opt/Packet.cpp:38-40
 *     and from the receiver verify                          cpp/src/base/Receiver.cpp:203-206
 *                                                           cpp/src/opt/Receiver.cpp:208-211
 *   - struct PacketHeader {type, seqNum, length, checksum}   cpp/src/common/PacketHeader.hpp:5-10
 *
 * The reference calls crc32() once per packet on the CPU.  These entry points take
 * whole batches of payloads that are already device-resident (or host buffers, for
 * the *_host_* wrappers) and compute every CRC in one HIP launch.  Results are
 * bit-identical to the reference: IEEE CRC-32, reflected polynomial 0xEDB88320,
 * init 0xFFFFFFFF, xorout 0xFFFFFFFF; crc of an empty payload is 0.
 *
 * Conventions
 *   - Plain pointers and sizes; `stream` is a hipStream_t passed as void* (NULL =
 *     the null stream).  Device entry points are asynchronous on that stream; the
 *     library keeps no pointer past stream completion.
 *   - Return 0 (WTP_OK) on success, a negative wtp_status on failure; never abort.
 *     wtp_last_error() gives a per-thread message for the last failure.
 *   - n == 0 is valid (no launch).  DATA payloads are at most WTP_MAX_PAYLOAD
 *     (1456 = 1500 - 20 IP - 8 UDP - 16 header, README.md:46-47); the kernels accept
 *     any payload up to WTP_MAX_KERNEL_LEN (4096 >= the 1484 bytes a 1500-byte
 *     recvfrom buffer can carry after the header, cpp/src/base/Receiver.cpp:123).
 *   - Device-side data errors (a length > WTP_MAX_KERNEL_LEN in a device array)
 *     cannot be returned by an async call: such packets get crc 0 and set a sticky
 *     per-device flag readable with wtp_device_status().
 */
#ifndef WTP_CRC32_H
#define WTP_CRC32_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WTP_MAX_PAYLOAD 1456u   /* cpp/src/base/Sender.cpp:20 CHUNK_SIZE */
#define WTP_MAX_KERNEL_LEN 4096u
#define WTP_HEADER_BYTES 16u    /* sizeof(PacketHeader), PacketHeader.hpp:5-10 */
#define WTP_TYPE_START 0u       /* cpp/src/base/Packet.hpp:8-13 */
#define WTP_TYPE_END 1u
#define WTP_TYPE_DATA 2u
#define WTP_TYPE_ACK 3u

typedef enum wtp_status {
    WTP_OK = 0,
    WTP_EINVAL = -1,   /* bad argument (null pointer with n > 0, length > max, ...) */
    WTP_EHIP = -2,     /* a HIP runtime call failed */
    WTP_ENOMEM = -3,   /* device or pinned allocation failed */
    WTP_ENODEV = -4    /* no usable gfx950 device */
} wtp_status;

/* Library version string. */
const char *wtp_version(void);

/* Message for the calling thread's last failure ("" if none). */
const char *wtp_last_error(void);

/* Kernel instantiation the calling thread's last launch used, e.g.
   "k_fixed_braid<6, 0, CrcHoldBEpi>" ("" if none).  Diagnostics: bench.py names the
   kernel its roofline measures with it. */
const char *wtp_last_kernel(void);

/* Number of visible HIP devices (0 when none). Does not create a context. */
int wtp_device_count(void);

/* Build the per-device constant tables for `device` now (they are otherwise built
   lazily on first use).  Call before capturing a launch into a hipGraph. */
int wtp_init(int device);

/* Leave `ncus` compute units of `device` free of the library's persistent kernels
   (0 <= ncus < the device's CUs; 0, the default, uses all).  For callers that overlap
   RCCL collectives with CRC launches, e.g. the gather of one batch's results with the
   next batch: a braided workgroup holds all of its CU's LDS, so a collective's
   workgroups can only start on CUs the launch leaves free.  Affects later launches on
   that device from any thread. */
int wtp_reserve_cus(int device, int ncus);

/* Sticky device-side flags of `device`.  Data errors: bit 0, a general-kernel payload
   length was > WTP_MAX_KERNEL_LEN (that payload's result is then 0 / not ok); bit 2, see
   wtp_crc32_verify_batch.  Informational: bit 3, the stream kernel met payloads that
   were not packed (or >= 4096 B) and computed them on its slower per-payload path
   (results exact).  Synchronous; clears the flags when `clear` != 0. */
int wtp_device_status(int device, uint32_t *flags, int clear);

/* ---- CPU reference semantics (single packet) --------------------------------------
   Replaces crc32() of cpp/src/common/Crc32.hpp:91-102 for single packets and 0-byte
   ACK payloads (Sender::isAckValid, cpp/src/base/Sender.cpp:235-237).  Pure C++
   byte-at-a-time table loop; thread-safe. */
uint32_t wtp_crc32(const void *buf, size_t size);

/* ---- device-resident batches (the hot path) ---------------------------------------
   Sender packet build, batched: payload i = d_payloads[i*stride .. i*stride+len).
   Replaces the per-chunk crc32 of Packet(DATA, chunk, seq) in the send loop
   (cpp/src/base/Sender.cpp:88-95 -> Packet.cpp:13).  Fast path (braided CDNA4
   kernel): base % 16 == 0, stride % 16 == 0, len % 16 == 0, 16 <= len <= 1536,
   stride <= 16384; other shapes run the general kernel (len <= WTP_MAX_KERNEL_LEN). */
int wtp_crc32_batch_fixed(const void *d_payloads, size_t stride, size_t len, size_t n,
                          uint32_t *d_out, void *stream);

/* Mixed lengths: payload i = d_base[d_offsets[i] .. d_offsets[i] + d_lengths[i]), any
   order, overlaps allowed.  `base_bytes` = size of the d_base buffer (bounds for the
   loads).  Buffers below 2 GiB run the general (piece-stream) kernel; larger ones take
   the route of wtp_crc32_batch_packed there (the piece kernel in device-cut < 2 GiB
   sub-launches, and the stream kernel, 64-bit offsets, for batches whose offsets turn
   out not to be packed), so there is no size limit.  d_lengths[i] <= WTP_MAX_KERNEL_LEN. */
int wtp_crc32_batch_var(const void *d_base, size_t base_bytes, const uint64_t *d_offsets,
                        const uint32_t *d_lengths, size_t n, uint32_t *d_out, void *stream);

/* Mixed lengths stored back to back (a receive buffer, a record file):
   d_offsets[i+1] == d_offsets[i] + d_lengths[i] (offsets = exclusive prefix sum of the
   lengths, any first offset).  The stream kernel: each wave hashes its region
   of the byte stream once and reads every payload's CRC off prefix values (no per-
   payload windows, masks or padding).  No limit on base_bytes (64-bit offsets) or n.
   Payloads that break the packing, or are longer than 4095 B, are still computed
   exactly on a slower lane-per-payload path, so results are correct for any offsets;
   lengths > WTP_MAX_KERNEL_LEN give crc 0 and set the status flag.
   The library picks the kernel: below 2 GiB the general kernel, the faster one on
   packed batches too (C5: DESIGN.md), so this call then equals wtp_crc32_batch_var; at
   or above 2 GiB the general kernel in sub-launches over < 2 GiB views that the device
   cuts from the offsets; a sub-launch that meets a payload outside its
   view (offsets not packed) flags it and the stream kernel then recomputes the batch,
   so results stay exact for any offsets.  That route keeps its descriptors in device
   scratch: 32 KiB per stream outside graph capture (made on the stream's first such
   call); a call captured into a graph takes one of 64 slots made at init, its own for
   the life of the process, so graphs captured on one stream may be replayed
   concurrently; with every slot taken a captured call runs the stream kernel (exact).
   WTP_STREAM_KERNEL=1 in the environment forces the stream kernel. */
int wtp_crc32_batch_packed(const void *d_base, size_t base_bytes, const uint64_t *d_offsets,
                           const uint32_t *d_lengths, size_t n, uint32_t *d_out, void *stream);

/* Receiver verify, batched (cpp/src/base/Receiver.cpp:25-35 + :203-206): datagram i is
   d_dgrams[i*stride .. i*stride + d_recv_len[i]) = 16-B big-endian PacketHeader ||
   payload.  As in the reference, the CRC covers bytes [16, recv_len) and
   header.length is ignored.  d_ok[i] = 1 iff 16 <= recv_len <= stride and
   ntohl(header.checksum) == crc32(payload), else 0 (drop, no ACK).  A recv_len
   above stride (more than the ring slot holds; recvfrom cannot return it) is
   malformed: ok 0.  d_crc_out may be NULL; otherwise it receives the computed CRCs
   (0 for runts and malformed lengths).  A payload above WTP_MAX_KERNEL_LEN bytes
   (recv_len - 16 > 4096, in a slot that holds it) is not hashed: ok 0, crc 0, and status
   bit 0 (wtp_device_status) is set.  Fast path: a 16-B aligned ring with
   stride % 16 == 0 (e.g. 1472 = header + 1456, or wReceiver's 1504-B slots holding the
   reference's 1500-B receive buffer) runs the braided kernel over the first
   min(stride - 16, 1456) payload bytes of every slot and decides the datagrams of
   exactly that length; in the same launch each workgroup then finishes its other
   datagrams (short, empty, 1473-1500 B, malformed) with the general algorithm.  The
   call uses no memory besides the caller's buffers and keeps no state between calls:
   graph captures, replays on any stream and concurrent calls are independent.  Status
   bit 2 (wtp_device_status): the recv_len array changed while the kernel ran. */
int wtp_crc32_verify_batch(const void *d_dgrams, size_t stride, const uint32_t *d_recv_len,
                           size_t n, uint8_t *d_ok, uint32_t *d_crc_out, void *stream);

/* Fused DATA packet builder (Packet.cpp:9-14,40-47 +
   Sender.cpp:187-197): chunk i = d_payloads[i*1456 ..) of min(1456, total-i*1456)
   bytes -> d_wire[i*wire_stride ..) = htonl{type=2, seq0+i, len, crc} || payload.
   wire_stride >= 16 + 1456.  d_wire_len[i] (may be NULL) = 16 + len. */
int wtp_build_data_packets(const void *d_payloads, size_t total_bytes, uint32_t seq0,
                           void *d_wire, size_t wire_stride, uint32_t *d_wire_len,
                           void *stream);

/* Fused DATA packet builder for mixed-length payloads, the sender-side counterpart of what
   wtp_accept_data_packets does for every length: payload i is d_base[d_offsets[i] ..
   + d_lengths[i]) (the layout of wtp_crc32_batch_var).  Payloads may be in any order and
   may overlap; offsets are full 64-bit and there is no size limit on base_bytes.  Payload
   i is valid iff d_lengths[i] <= WTP_MAX_PAYLOAD, d_offsets[i] <= base_bytes and
   d_lengths[i] <= base_bytes - d_offsets[i].  For a valid i, with len = d_lengths[i]:
   d_wire[i*wire_stride .. +16) = htonl{type = 2, seqNum = seq0 + i (mod 2^32), length =
   len, checksum = crc32(payload)} and the payload follows the header, byte-identical to
   oracle.build_datagram(seq0 + i, payload) (oracle/oracle.py) and, for a 1456-byte
   payload, to what wtp_build_data_packets writes; d_wire_len[i] = 16 + len and
   d_crc_out[i] = the checksum.  len == 0 is valid (checksum 0, wire length 16).  For an invalid i the slot
   is not written at all, d_wire_len[i] = 0 and d_crc_out[i] = 0; no status flag is set
   (as in wtp_tx_ingest_acks), so with d_wire_len == NULL nothing reports an invalid
   entry.  Nothing else is written: bytes [16 + len, wire_stride) of every slot and
   everything outside [d_wire, d_wire + n*wire_stride) stay as they were; d_base,
   d_offsets and d_lengths are only read, and no byte outside [d_base, d_base +
   base_bytes) is ever loaded, by the widened and aligned-down vector loads and for
   invalid payloads too (a vector at an edge of the buffer is loaded bytewise).  d_wire
   overlapping d_base is undefined.  d_wire_len and d_crc_out may be NULL.  n == 0 is
   valid and launches nothing.  WTP_EINVAL (before any device is touched): wire_stride <
   1472, n >= 2^31, a NULL d_base, d_offsets, d_lengths or d_wire with n > 0.  One
   stream-ordered launch with no host synchronisation, no allocation and no scratch; the
   call uses no memory besides the caller's buffers and keeps no state.  It reads no
   library table, so it needs no wtp_init before a capture; graph captures, replays and
   concurrent calls are independent.  wtp_last_kernel() names "k_build_var".  Fast path
   (16-B vector stores, each payload byte read once: the kernel hashes what it copies): a
   16-B aligned d_wire with wire_stride % 16 == 0, and any source alignment (packed
   payloads sit at arbitrary byte addresses); other wire alignments are built bytewise,
   exactly. */
int wtp_build_data_packets_var(const void *d_base, size_t base_bytes,
                               const uint64_t *d_offsets, const uint32_t *d_lengths, size_t n,
                               uint32_t seq0, void *d_wire, size_t wire_stride,
                               uint32_t *d_wire_len, uint32_t *d_crc_out, void *stream);

/* Device-side receive, the inverse of wtp_build_data_packets: verify, window-place and
   ACK a batch of datagrams (cpp/src/base/Receiver.cpp:25-35 payload memcpy + :208-237
   window check, buffering, next_seq).  Datagrams as in wtp_crc32_verify_batch.  The
   caller owns the window state, which persists across calls: d_out, window * 1456 bytes,
   the file image from chunk seq0 on (slot s = bytes [s*1456, (s+1)*1456)), and
   d_slot_len[window], WTP_SLOT_EMPTY for an empty slot, else the payload length stored
   in it (set it to 0xFF bytes once; shift or reset it when the window advances:
   wtp_rx_advance below does that on the device).  On entry every d_slot_len value must be
   WTP_SLOT_EMPTY or below 0x80000000: any such value other than WTP_SLOT_EMPTY counts as
   filled (for placing and for the ACK alike) and is carried unchanged, whether or not it
   is a possible payload length.  Values in [0x80000000, 0xFFFFFFFF) are the call's own
   transient claims (0x80000000 | datagram index) and are not valid input: a datagram may
   be placed over one.  A completed call leaves none behind.
   The result equals processing the datagrams one by one in index (arrival) order:
   d_ok[i] is what wtp_crc32_verify_batch writes.  Datagram i is placed iff d_ok[i],
   ntohl(type) == WTP_TYPE_DATA, len = recv_len - 16 <= WTP_MAX_PAYLOAD,
   s = ntohl(seqNum) - seq0 (unsigned 32-bit, so a wrapping window is well defined)
   < window, slot s was empty on entry and no placed datagram of a lower index carries
   the same seqNum (first arrival wins).  Then d_out[s*1456 .. +len) = payload,
   d_slot_len[s] = len (0 for an empty payload) and d_place[i] = s; otherwise d_place[i]
   = WTP_NOT_PLACED.  Nothing else in d_out or d_slot_len changes: bytes [len, 1456) of
   a placed slot, slots that receive nothing, and all of d_out for a corrupt datagram
   stay as they were; a slot never mixes two datagrams' bytes.  *d_ack = seq0 + the number
   of leading non-empty slots after the call (the cumulative ACK).  d_place and d_ack may
   be NULL.  n == 0 and window == 0 are valid; with n == 0, *d_ack is still written from
   the existing state.  WTP_EINVAL (before any device is touched): a NULL d_dgrams,
   d_recv_len, d_ok, d_out or d_slot_len with n > 0, stride < 16, n >= 2^31.  Fast copy
   (16-B vectors), chosen per datagram: a payload whose address in the ring and whose slot
   in d_out are both 16-B aligned (every datagram of a 16-B aligned ring with stride % 16
   == 0 and a 16-B aligned d_out); any other datagram is copied bytewise.
   Stream-ordered launches (verify, claim, place) with no host synchronisation; the call
   uses no memory besides the caller's buffers (slots are claimed in d_slot_len itself)
   and keeps no state: graph captures, replays and concurrent calls on different windows
   are independent. */
#define WTP_SLOT_EMPTY 0xFFFFFFFFu
#define WTP_NOT_PLACED 0xFFFFFFFFu
int wtp_accept_data_packets(const void *d_dgrams, size_t stride, const uint32_t *d_recv_len, size_t n,
                            uint32_t seq0, uint32_t window,
                            void *d_out, uint32_t *d_slot_len,
                            uint8_t *d_ok, uint32_t *d_place, uint32_t *d_ack, void *stream);

/* ---- device-side sender window: ACK ingest and selective retransmit ----------------
   The mirror of wtp_accept_data_packets.  The caller owns the window state, which persists
   across calls: slot s in [0, inflight) is the DATA packet with seqNum seq0 + s (unsigned
   32-bit, so a wrapping window is well defined), d_acked[s] is 0 or 1, d_sent_ms[s] is the
   caller's millisecond clock at that packet's last send (it wraps at 2^32).  d_payloads
   points at the first byte of chunk seq0 and total_bytes is the number of file bytes from
   there on: slot s holds min(1456, total_bytes - s*1456) bytes.  When the window advances
   by a, the caller shifts d_acked and d_sent_ms by a and moves d_payloads, total_bytes and
   seq0.  wtp_tx_advance below does that shift on the device.  inflight <=
   WTP_TX_MAX_INFLIGHT.

   wtp_tx_ingest_acks turns a batch of received datagrams (laid out as in
   wtp_crc32_verify_batch) into window state.  d_ok[i] is what wtp_crc32_verify_batch
   writes (for a plain 16-byte ACK: checksum == 0, decided without hashing; a longer
   datagram is hashed exactly; a payload above WTP_MAX_KERNEL_LEN is not ok, as there,
   but this call does not set the status flag).  WTP_ACK_SELECTIVE (cpp/src/opt/
   Sender.cpp:130-139, Window.cpp:45-54): datagram i counts iff d_ok[i], ntohl(type) ==
   WTP_TYPE_ACK and s = ntohl(seqNum) - seq0 < inflight; then d_acked[s] = 1 and d_hit[i]
   = s.  WTP_ACK_CUMULATIVE (cpp/src/base/Sender.cpp:107-109): it counts iff ok, of type
   ACK and a = ntohl(seqNum) - seq0 has 0 < a <= inflight; then d_hit[i] = a, and
   d_acked[s] = 1 for every s < the largest a of the batch.  Every other datagram gets
   d_hit[i] = WTP_NOT_PLACED.  d_counts[0] = the number of leading slots with d_acked != 0
   after the call (the window advance, Window.cpp:66-75), d_counts[1] = the number of
   slots that went 0 -> 1 in this call; nothing else in d_acked changes.  The result
   equals processing the datagrams one by one in index order.  d_hit may be NULL.  n == 0
   and inflight == 0 are valid: d_counts is still written from the existing state.
   n >= 2^31, inflight > WTP_TX_MAX_INFLIGHT, an unknown mode, stride < 16 or a NULL
   required pointer (d_counts; d_acked with inflight > 0; d_dgrams, d_recv_len, d_ok with
   n > 0) returns WTP_EINVAL before any device is touched.  Stream-ordered (a memset of
   d_counts, one lane per datagram, one pass over the window), no host
   synchronisation; the call uses no memory besides the caller's buffers and keeps no
   state: graph captures, replays and concurrent calls on different windows are
   independent. */
#define WTP_ACK_SELECTIVE  0u   /* opt/Sender.cpp:130-139: an ACK names the one packet it acknowledges */
#define WTP_ACK_CUMULATIVE 1u   /* base/Sender.cpp:107-109: an ACK names the next expected packet */
#define WTP_RETX_ALL       1u   /* flags: every un-ACKed slot is due, timers ignored (go-back-N) */
#define WTP_TX_MAX_INFLIGHT (1u << 20)
int wtp_tx_ingest_acks(const void *d_dgrams, size_t stride, const uint32_t *d_recv_len, size_t n,
                       uint32_t mode, uint32_t seq0, uint32_t inflight, uint32_t *d_acked,
                       uint8_t *d_ok, uint32_t *d_hit, uint32_t *d_counts, void *stream);

/* wtp_tx_build_retransmit selects the slots that are due and builds exactly those
   datagrams again (cpp/src/opt/Sender.cpp:121-127, Packet.cpp:52-56; with WTP_RETX_ALL
   cpp/src/base/Sender.cpp:101-105).  Slot s is due iff d_acked[s] == 0 and (flags &
   WTP_RETX_ALL or (uint32_t)(now_ms - d_sent_ms[s]) > timeout_ms).  Due slots are taken in
   rising slot order and the first min(due, max_sel) of them are emitted: entry k gets
   d_sel[k] = s, d_wire[k*wire_stride ..) = htonl{type = 2, seq0 + s, len, crc32(payload)}
   || payload, byte-identical to what wtp_build_data_packets writes for that chunk,
   d_wire_len[k] = 16 + len, and d_sent_ms[s] = now_ms.  d_counts[0] = the number emitted,
   d_counts[1] = the number due (a caller whose ring was too small calls again).  Entries
   k >= d_counts[0] of d_wire, d_sel and d_wire_len and the timers of slots not emitted stay
   as they were; d_acked and d_payloads are only read.  d_sel and d_wire_len may be NULL.
   inflight == 0 and max_sel == 0 are valid: d_counts is still written.  WTP_EINVAL (before
   any device is touched): wire_stride < 1472, inflight > WTP_TX_MAX_INFLIGHT (the
   window's bytes stay below 2 GiB),
   (inflight - 1) * 1456 >= total_bytes with inflight > 0, work_bytes <
   wtp_tx_work_bytes(inflight, max_sel), a NULL d_counts or d_work, a NULL d_payloads,
   d_acked or d_sent_ms with inflight > 0, a NULL d_wire with inflight and max_sel > 0.
   d_work is the caller's scratch as for wtp_crc32_concat (any alignment, contents
   arbitrary on entry, unspecified on return, no allocation by the library);
   wtp_tx_work_bytes is monotone in both arguments and at most 64 KiB + 16 bytes per
   max_sel entry.  Fast path (16-B vectors, each payload byte read once: the emit kernel
   hashes what it copies): 16-B aligned d_payloads and d_wire with wire_stride % 16 == 0;
   other alignments, and a chunk shorter than 1456 bytes, are copied and hashed bytewise,
   exactly.  Stream-ordered launches (count, select, emit) with no host synchronisation:
   d_counts[0] is never read on the host, grids are sized from max_sel.  The call reads no
   library table, so it needs no wtp_init before a capture.  wtp_last_kernel() names
   "k_tx_emit" (or "k_tx_select" when max_sel or inflight is 0 and nothing can be
   emitted). */
size_t wtp_tx_work_bytes(uint32_t inflight, uint32_t max_sel);
int wtp_tx_build_retransmit(const void *d_payloads, size_t total_bytes, uint32_t seq0, uint32_t inflight,
                            const uint32_t *d_acked, uint32_t *d_sent_ms, uint32_t now_ms,
                            uint32_t timeout_ms, uint32_t flags,
                            void *d_wire, size_t wire_stride, uint32_t max_sel,
                            uint32_t *d_sel, uint32_t *d_wire_len, uint32_t *d_counts,
                            void *d_work, size_t work_bytes, void *stream);

/* wtp_tx_build_retransmit_var is wtp_tx_build_retransmit for records of mixed length, in the
   layout of wtp_crc32_batch_var and wtp_build_data_packets_var (base, offsets, lengths).
   The window state (d_acked, d_sent_ms, seq0, inflight, the due rule, flags) is exactly
   that of wtp_tx_build_retransmit.  Slot s in [0, inflight) is the record d_base[
   d_offsets[s] .. + d_lengths[s]).  d_offsets and d_lengths are passed already advanced to
   the window base: when the window advances by a, the caller adds a to the two pointers
   and to seq0.  d_base and base_bytes stay the whole buffer: they bound the loads, as in
   wtp_build_data_packets_var.  No entry at or above inflight of either array is read.
   Offsets are full 64-bit, records may be in any order and may overlap, and there is no
   size limit on base_bytes.
   Selection is that of wtp_tx_build_retransmit, word for word: slot s is due iff
   d_acked[s] == 0 and (flags & WTP_RETX_ALL or (uint32_t)(now_ms - d_sent_ms[s]) >
   timeout_ms); due slots are taken in rising slot order and the first min(due, max_sel) of
   them are emitted, entry k gets d_sel[k] = s and d_sent_ms[s] = now_ms; d_counts[0] = the
   number emitted, d_counts[1] = the number due.  The selection does not look at the
   records: a due slot whose record is invalid is still selected, still counted and still
   gets its timer reset.
   Emit: entry k with s = d_sel[k] follows wtp_build_data_packets_var's rule for one
   payload.  It is valid iff len = d_lengths[s] <= WTP_MAX_PAYLOAD, off = d_offsets[s] <=
   base_bytes and len <= base_bytes - off.  A valid entry writes d_wire[k*wire_stride ..) =
   htonl{type = 2, seqNum = seq0 + s (mod 2^32), length = len, checksum = crc32(payload)}
   || payload, d_wire_len[k] = 16 + len and d_crc_out[k] = the checksum.  The datagram is
   byte-identical to oracle.build_datagram(seq0 + s, payload) (oracle/oracle.py), to what
   wtp_build_data_packets_var writes for that record and, for a 1456-byte chunk, to what
   wtp_tx_build_retransmit writes.  len == 0 is valid (checksum 0, wire length 16).  For an
   invalid entry the slot is not written at all, d_wire_len[k] = 0 and d_crc_out[k] = 0.
   Nothing else is written: entries k >= d_counts[0] of d_wire, d_sel, d_wire_len and
   d_crc_out, bytes [16 + len, wire_stride) of every slot and the timers of slots not
   emitted stay as they were; d_base, d_offsets, d_lengths and d_acked are only read, and
   no byte outside [d_base, d_base + base_bytes) is ever loaded (a vector at an edge of the
   buffer is loaded bytewise, as in the builder).  d_wire overlapping d_base is undefined.
   d_sel, d_wire_len and d_crc_out may be NULL.  inflight == 0 and max_sel == 0 are valid:
   d_counts is still written.
   WTP_EINVAL (before any device is touched, each with its own message): wire_stride <
   1472, inflight > WTP_TX_MAX_INFLIGHT, work_bytes < wtp_tx_work_bytes(inflight, max_sel)
   (the same function and the same scratch contract as wtp_tx_build_retransmit), a NULL
   d_counts or d_work, a NULL d_base, d_offsets, d_lengths, d_acked or d_sent_ms with
   inflight > 0, a NULL d_wire with inflight > 0 and max_sel > 0.  There is no total_bytes
   check: validity is per record, on the device.
   Stream-ordered launches (count, select, emit) with no host synchronisation and no
   allocation: d_counts[0] is never read on the host, grids are sized from max_sel (the
   emit kernel reads the count on the device and spreads the emitted datagrams over its
   grid, so a small due set costs the same in a large ring as in a fitted one).  The call
   reads no library table, so it needs no wtp_init before a capture; captures, replays and
   concurrent calls on different work buffers are independent.  wtp_last_kernel() names
   "k_tx_emit_var" (or "k_tx_select" when max_sel or inflight is 0).  Fast path: a 16-B
   aligned d_wire with wire_stride % 16 == 0 and any source alignment; other wire
   alignments are built bytewise, exactly. */
int wtp_tx_build_retransmit_var(const void *d_base, size_t base_bytes,
                                const uint64_t *d_offsets, const uint32_t *d_lengths,
                                uint32_t seq0, uint32_t inflight,
                                const uint32_t *d_acked, uint32_t *d_sent_ms, uint32_t now_ms,
                                uint32_t timeout_ms, uint32_t flags,
                                void *d_wire, size_t wire_stride, uint32_t max_sel,
                                uint32_t *d_sel, uint32_t *d_wire_len, uint32_t *d_crc_out,
                                uint32_t *d_counts, void *d_work, size_t work_bytes, void *stream);

/* ---- device-side ACK generation: the receiver's reply ring ---------------------------
   The fourth call of the protocol loop: it follows wtp_accept_data_packets on the same
   stream, takes the same batch (datagrams as in wtp_crc32_verify_batch), seq0 and window,
   accept's outputs d_ok and d_place and the window state d_slot_len after that call, and
   writes the ACK datagrams the receiver owes, ready for the sender's wtp_tx_ingest_acks.
   The window is fixed for the batch, as in accept.  The result equals processing the
   datagrams one by one in index order.

   Eligibility, the same in both modes: datagram i is answered iff d_ok[i] != 0,
   ntohl(type) == WTP_TYPE_DATA, recv_len[i] - 16 <= WTP_MAX_PAYLOAD and, with d =
   ntohl(seqNum) - seq0 in unsigned 32-bit arithmetic, d < window or d >= 0x80000000.  The
   second case is a packet below the window: its ACK was lost, the sender re-sent it after
   the receiver had moved on, and it must be ACKed again or the sender never finishes
   (cpp/src/opt/Receiver.cpp:211-237 and cpp/src/base/Receiver.cpp:206-237 answer every
   intact datagram they do not drop; wReceiver.cpp answers below `expected`).  An intact
   in-window datagram that accept did not place because its slot was already full (a
   duplicate, or the loser of the first-wins race) is still answered.  A datagram at or
   above seq0 + window, a corrupt one, a runt, a payload above 1456 bytes and a type other
   than DATA are not.

   The ACK's seqNum.  WTP_ACK_SELECTIVE (opt/Receiver.cpp:213,227): the datagram's own
   seqNum; d_place and d_slot_len are not read and may be NULL.  WTP_ACK_CUMULATIVE
   (base/Receiver.cpp:213-227; wReceiver.cpp `ack_seq = expected`): seq0 + lead_i, where
   lead_i is the number of leading non-empty slots after datagrams 0 .. i have been
   processed in order.  Every slot s of the window has a fill time: j, the lowest index
   with d_place[j] == s, if there is one; else -1 if d_slot_len[s] != WTP_SLOT_EMPTY (it was
   filled before the batch); else never.  lead_i is the length of the leading run of slots
   with fill time <= i.  A d_place entry >= window counts as WTP_NOT_PLACED, so any input is
   defined and nothing is indexed outside the window.  With accept's own outputs seq0 +
   lead_(n-1) equals accept's *d_ack.  Datagrams below the window carry the running value
   too.

   Output.  The eligible datagrams are ranked in rising index (arrival) order; those with
   rank r in [skip, skip + max_acks) are emitted as entry k = r - skip:
   d_ack_wire[k*ack_stride .. +16) = htonl{type = 3, seqNum, length = 0, checksum = 0}
   (crc32 of the empty payload is 0) and d_src[k] = i.  d_counts[0] = the number emitted,
   d_counts[1] = the number eligible; a caller whose ring was too small calls again with
   skip += max_acks.  Entries k >= d_counts[0] of d_ack_wire and d_src and bytes [16,
   ack_stride) of every slot stay as they were; every input is only read.  d_src may be
   NULL.  n == 0, window == 0 and max_acks == 0 are valid: d_counts is still written.

   WTP_EINVAL (before any device is touched): n > WTP_RX_MAX_BATCH, window >
   WTP_RX_MAX_WINDOW in cumulative mode, an unknown mode, stride < 16, ack_stride < 16,
   work_bytes < wtp_rx_ack_work_bytes(n, window, mode), a NULL d_counts or d_work, a NULL
   d_dgrams, d_recv_len or d_ok with n > 0, a NULL d_place or d_slot_len in cumulative mode
   with n > 0 and window > 0, a NULL d_ack_wire with n > 0 and max_acks > 0.

   d_work is the caller's scratch as for wtp_tx_build_retransmit (any alignment, contents
   arbitrary on entry, unspecified on return, no allocation by the library; every word the
   call reads it has written before).  wtp_rx_ack_work_bytes is monotone in n and window
   and at most 64 KiB + 4 bytes per 1024 datagrams + 4 bytes per window slot (the window
   term in cumulative mode only).  The header is one 16-byte store where the slot is 16-B
   aligned (every slot of a 16-B aligned ring with ack_stride % 16 == 0), bytes otherwise.
   Stream-ordered launches (selective: mark, emit; cumulative: init, mark, block maxima,
   scan, emit) with no host synchronisation: d_counts[0] is never read on the host, grids
   are sized from n and window.  The call keeps no state and reads no library table, so it
   needs no wtp_init before a capture, and concurrent calls on different work buffers are
   independent.  wtp_last_kernel() names "k_ack_emit". */
#define WTP_RX_MAX_WINDOW (1u << 20)   /* cumulative mode only; wtp_rx_deliver */
#define WTP_RX_MAX_BATCH  (1u << 24)
size_t wtp_rx_ack_work_bytes(size_t n, uint32_t window, uint32_t mode);
int wtp_rx_build_acks(const void *d_dgrams, size_t stride, const uint32_t *d_recv_len, size_t n,
                      uint32_t mode, uint32_t seq0, uint32_t window,
                      const uint8_t *d_ok, const uint32_t *d_place, const uint32_t *d_slot_len,
                      void *d_ack_wire, size_t ack_stride, uint32_t skip, uint32_t max_acks,
                      uint32_t *d_src, uint32_t *d_counts,
                      void *d_work, size_t work_bytes, void *stream);

/* ---- multi-connection receive: accept and ACK one batch across flows ------------------
   wtp_accept_data_packets and wtp_rx_build_acks for a receiver with many concurrent
   senders: one batch holds the arrivals of all connections, interleaved in arrival order
   (what recvmmsg returns), and one call serves every connection's window.  Per-connection
   semantics are exactly those of the two calls above (the reference serves one connection
   at a time and drops a second START, cpp/src/opt/Receiver.cpp:145-150); only the
   batching across connections is new.

   State.  All flows share one `window`, the receiver's parameter.  Flow f in [0, nflows)
   owns slots [f*window, (f+1)*window) of one d_slot_len[nflows*window] and one image d_out
   of nflows*window*1456 bytes: its sub-window is d_out + f*window*1456, d_slot_len +
   f*window, which is the state wtp_accept_data_packets, wtp_rx_deliver and wtp_rx_advance
   take, so those calls work on one flow unchanged; wtp_rx_deliver_flows and
   wtp_rx_advance_flows below flush and slide all flows at once.  d_seq0[nflows] (device
   memory, read when the kernels run) is each flow's window base: wtp_rx_advance_flows (or the
   host) moves it between rounds, and one captured graph serves every round.  d_flow[n] (device)
   names each datagram's flow, derived by the caller from the datagram's source address;
   any value >= nflows means "no connection".

   wtp_accept_data_packets_flows.  The result equals processing the datagrams one by one in
   index (arrival) order, each against its own flow's window; equivalently, for every flow
   f it is what wtp_accept_data_packets gives on the subsequence of datagrams with d_flow[i]
   == f, in index order, against flow f's sub-window with seq0 = d_seq0[f].  d_ok[i] is what
   wtp_crc32_verify_batch writes, for every datagram ("no connection" ones included).
   Datagram i is placed iff d_ok[i], f = d_flow[i] < nflows, ntohl(type) == WTP_TYPE_DATA,
   len = recv_len - 16 <= WTP_MAX_PAYLOAD, s = ntohl(seqNum) - d_seq0[f] (unsigned 32-bit, so
   a wrapping window is well defined) < window, slot f*window + s was empty on entry and no
   placed datagram of a lower index and the same flow carries the same seqNum (first arrival
   wins).  Then d_out[(f*window + s)*1456 .. +len) = payload, d_slot_len[f*window + s] = len
   and d_place[i] = s, the slot within the flow (so nflows == 1 reproduces
   wtp_accept_data_packets word for word); otherwise d_place[i] = WTP_NOT_PLACED.  The same
   seqNum in two flows never collides.  d_ack[f] = d_seq0[f] + the number of leading
   non-empty slots of flow f after the call, written for every f < nflows, also with n == 0
   and for a flow that no datagram names.  As in wtp_accept_data_packets: on entry every
   d_slot_len value is WTP_SLOT_EMPTY or below 0x80000000, values in [0x80000000, 0xFFFFFFFF)
   are the call's transient claims (0x80000000 | datagram index) and a completed call leaves
   none behind; nothing else in d_out or d_slot_len changes; a slot never mixes two
   datagrams' bytes; the inputs are only read; the copy is 16-B vectors for a datagram
   whose payload address and slot are both 16-B aligned, bytes otherwise (1456 = 91 * 16, so
   a 16-B aligned d_out keeps every flow's slots aligned).  d_place and d_ack may be NULL.
   n == 0, nflows == 0 and window == 0 are valid.
   WTP_EINVAL (before any device is touched, each with its own message): n >= 2^31, stride <
   16, nflows > WTP_RX_MAX_FLOWS, window > WTP_RX_MAX_WINDOW, nflows * window (in 64 bits) >
   WTP_RX_MAX_FLOW_SLOTS, a NULL d_dgrams, d_recv_len, d_flow, d_ok, d_out or d_slot_len with
   n > 0, a NULL d_seq0 with nflows > 0 and (n > 0 or d_ack).
   Stream-ordered launches (verify, claim, place + per-flow ACK) with no host
   synchronisation; no memory besides the caller's buffers (claims live in d_slot_len) and
   no library state: graph captures, replays and concurrent calls on different states are
   independent.  The per-flow ACK costs no launch and no serial walk per flow: all
   nflows*window slots are spread over the place kernel's grid, 2^20 flows of 16 slots and
   one flow of 2^20 slots alike.  wtp_last_kernel() names "k_flows_place".

   wtp_rx_build_acks_flows follows it on the same stream with the same batch, d_flow, d_seq0
   values, nflows and window, accept's d_ok and (in cumulative mode) its d_ack as d_flow_ack.
   Eligibility is wtp_rx_build_acks' rule with the flow's base: datagram i is answered iff
   d_ok[i] != 0, f = d_flow[i] < nflows, ntohl(type) == WTP_TYPE_DATA, recv_len[i] - 16 <=
   WTP_MAX_PAYLOAD and, with d = ntohl(seqNum) - d_seq0[f], d < window or d >= 0x80000000.
   The ACK's seqNum: WTP_ACK_SELECTIVE, the datagram's own seqNum (d_flow_ack is not read
   and may be NULL); WTP_ACK_CUMULATIVE, d_flow_ack[f], the flow's cumulative ACK after the
   whole batch.  This differs from wtp_rx_build_acks, which gives the running value after
   each arrival: a cumulative ACK that names a later next-expected packet is always valid,
   and the sender's wtp_tx_ingest_acks takes the batch maximum anyway; the running value
   across flows is a segmented prefix problem and is not computed here.
   Output as in wtp_rx_build_acks: the eligible datagrams are ranked in arrival order, those
   of rank r in [skip, skip + max_acks) become entry k = r - skip of d_ack_wire (16 bytes,
   ack_stride apart) with d_src[k] = i (the reply address is that of d_flow[d_src[k]]);
   d_counts = {emitted, eligible}; entries past d_counts[0], bytes [16, ack_stride) of every
   slot and every input stay as they were; d_src may be NULL; one 16-B store per 16-B
   aligned slot, bytes otherwise.  n == 0, nflows == 0, window == 0 and max_acks == 0 are
   valid: d_counts is still written.  d_work is scratch as in wtp_rx_build_acks (any
   alignment); wtp_rx_ack_flows_work_bytes is monotone in n and at most 64 KiB + 4 bytes per
   1024 datagrams.
   WTP_EINVAL (before any device is touched): n > WTP_RX_MAX_BATCH, an unknown mode, window >
   WTP_RX_MAX_WINDOW in cumulative mode, stride < 16, ack_stride < 16, work_bytes <
   wtp_rx_ack_flows_work_bytes(n), a NULL d_counts or d_work; with n > 0, a NULL d_dgrams,
   d_recv_len, d_ok or d_flow, a NULL d_seq0 with nflows > 0, a NULL d_flow_ack in cumulative
   mode with nflows > 0, a NULL d_ack_wire with max_acks > 0.
   Stream-ordered launches (mark, emit), no host synchronisation, no state, no library
   table: no wtp_init is needed before a capture.  wtp_last_kernel() names
   "k_flows_ack_emit". */
#define WTP_RX_MAX_FLOWS      (1u << 20)
#define WTP_RX_MAX_FLOW_SLOTS (1u << 24)   /* nflows * window */
int wtp_accept_data_packets_flows(const void *d_dgrams, size_t stride, const uint32_t *d_recv_len,
                                  const uint32_t *d_flow, size_t n,
                                  const uint32_t *d_seq0, uint32_t nflows, uint32_t window,
                                  void *d_out, uint32_t *d_slot_len,
                                  uint8_t *d_ok, uint32_t *d_place, uint32_t *d_ack, void *stream);
size_t wtp_rx_ack_flows_work_bytes(size_t n);
int wtp_rx_build_acks_flows(const void *d_dgrams, size_t stride, const uint32_t *d_recv_len,
                            const uint32_t *d_flow, size_t n, uint32_t mode,
                            const uint32_t *d_seq0, uint32_t nflows, uint32_t window,
                            const uint8_t *d_ok, const uint32_t *d_flow_ack,
                            void *d_ack_wire, size_t ack_stride, uint32_t skip, uint32_t max_acks,
                            uint32_t *d_src, uint32_t *d_counts,
                            void *d_work, size_t work_bytes, void *stream);

/* ---- in-order flush: the window's leading run as a packed stream ---------------------
   The sixth call of the protocol loop (cpp/src/base/Receiver.cpp:208-237, the in-order
   flush; wReceiver.cpp's std::map loop): it follows wtp_accept_data_packets and
   wtp_rx_build_acks and turns the in-order prefix of the window back into the byte stream
   the sender started from, in the (base, offsets, lengths) layout of wtp_crc32_batch_var, so
   that packed records -> wtp_build_data_packets_var -> channel -> wtp_accept_data_packets
   -> wtp_rx_deliver gives the same packed records, and wtp_crc32_batch_packed,
   wtp_crc32_buffer and wtp_crc32_concat apply to the output directly.

   d_img and d_slot_len are accept's window state (its d_out and d_slot_len), passed already
   offset to the current window base: slot s = d_img[s*1456 .. +1456), d_slot_len[s] its
   stored length or WTP_SLOT_EMPTY.  run = the number of leading slots with d_slot_len[s] <=
   WTP_MAX_PAYLOAD: any larger value (WTP_SLOT_EMPTY, a claim pattern 0x80000000 | i,
   anything else) ends the run, so every input is defined and nothing is indexed by a bad
   length.  P_s = the sum of d_slot_len[t] for t < s (64-bit).  k = the largest value with k
   <= min(run, max_slots) and stream_off + P_k <= stream_bytes: whole records only, and
   zero-length records that still fit are included.  For s < k, with len = d_slot_len[s]:
   d_stream[stream_off + P_s .. + len) = d_img[s*1456 .. + len), d_offsets_out[s] =
   stream_off + P_s and d_lengths_out[s] = len.  d_counts[0] = k, d_counts[1] = run,
   d_counts[2] = P_k (the bytes delivered), d_counts[3] = P_run (the bytes the whole run
   needs: a caller whose buffer was too small sizes the next one from it).  d_counts is
   always written, also for window == 0 and max_slots == 0, which are both valid; with
   max_slots == 0, run and P_run are still reported.

   Nothing else is written: every byte of d_stream outside [stream_off, stream_off + P_k)
   stays as it was, the bytes that share a 16-B vector with the first and the last
   delivered byte included (no read-modify-write of neighbouring bytes); entries >= k of
   d_offsets_out and d_lengths_out stay as they were; d_img and d_slot_len are only read
   (the caller resets or shifts them when it advances the window by k, as today;
   wtp_rx_advance below takes d_counts as it is and does that on the device), and no
   byte outside [d_img, d_img + window*1456) is ever loaded, by the widened and aligned-down
   vector loads at the image's two ends too.  d_stream overlapping d_img is undefined.
   d_offsets_out and d_lengths_out may be NULL.

   WTP_EINVAL (before any device is touched): window > WTP_RX_MAX_WINDOW (so P < 2^31),
   stream_off > stream_bytes, work_bytes < wtp_rx_deliver_work_bytes(window), a NULL d_counts
   or d_work, a NULL d_img or d_slot_len with window > 0, a NULL d_stream with window > 0
   and max_slots > 0.

   d_work is the caller's scratch as for wtp_rx_build_acks (any alignment, contents
   arbitrary on entry, unspecified on return, no allocation by the library; every word the
   call reads it has written before).  wtp_rx_deliver_work_bytes is monotone and at most
   64 KiB + 8 bytes per window slot.  Fast path (one 16-B store per 16 stream bytes whatever
   the stream's byte phase, the source loaded as dwords and shifted): a 4-B aligned d_img;
   a vector that spans records, the first and last vector of the delivered range, a vector
   at the image's end and any other image alignment are gathered bytewise, exactly.
   Stream-ordered launches (block sums, scan, copy) with no host synchronisation: d_counts is
   never read on the host, grids are sized from window and max_slots.  No allocation and no
   library table, so no wtp_init is needed before a capture; graph captures, replays and
   concurrent calls on different work buffers are independent.  wtp_last_kernel() names
   "k_deliver_copy" (or "k_deliver_scan" when window or max_slots is 0 and nothing can be
   copied). */
size_t wtp_rx_deliver_work_bytes(uint32_t window);
int wtp_rx_deliver(const void *d_img, const uint32_t *d_slot_len, uint32_t window, uint32_t max_slots,
                   void *d_stream, size_t stream_bytes, uint64_t stream_off,
                   uint64_t *d_offsets_out, uint32_t *d_lengths_out, uint64_t *d_counts,
                   void *d_work, size_t work_bytes, void *stream);

/* ---- sliding both windows: the end of a round ------------------------------------------
   The six calls above each handle one batch against a window that is fixed for that batch;
   these two move the window.  A receive round is accept -> ACKs -> deliver -> advance, all
   stream-ordered with one host read at the end, and a transfer of any length runs in two
   windows' worth of state.  Both calls write a second copy of the state: the caller keeps
   two sets of buffers and swaps them each round (an in-place slide would make every slot
   both a source and a destination of workgroups that run in no defined order).

   wtp_rx_advance slides accept's window state (d_img, window * 1456 bytes, and d_slot_len,
   as in wtp_rx_deliver) down by a slots into d_img_next / d_slot_len_next.  d_adv points at
   one device-resident uint64_t, read on the device when the kernel runs, not when the call is
   made: wtp_rx_deliver's d_counts can be passed as it is (d_counts[0] = k) with no host read
   in between, and one captured graph serves every round.  a = min(*d_adv, window), compared
   in 64 bits, so any value of *d_adv is defined.  For every s in [0, window), with t = s + a
   and v = d_slot_len[t] if t < window, else WTP_SLOT_EMPTY: d_slot_len_next[s] = v, for
   every v (a value above WTP_MAX_PAYLOAD, that is WTP_SLOT_EMPTY, a claim pattern or anything
   else, is carried unchanged and nothing is copied for it); and if v <= WTP_MAX_PAYLOAD and
   the images are given, d_img_next[s*1456 .. + v) = d_img[t*1456 .. + v).  Nothing else is
   written: bytes [v, 1456) of slot s in d_img_next stay as they were (accept's rule for a
   placed slot), a slot that receives no record stays whole, and no byte outside [d_img_next,
   d_img_next + window*1456) or [d_slot_len_next, + 4*window) is written.  d_img, d_slot_len
   and *d_adv are only read, and no byte outside [d_img, d_img + window*1456) is ever loaded,
   by the vector loads at the image's two ends too.  d_img and d_img_next may both be NULL:
   then only d_slot_len moves (a fixed-chunk transfer, where the image already is the file
   and the caller moves a pointer, not bytes).  window == 0 is valid and launches nothing.

   WTP_EINVAL (before any device is touched), each with its own message: window >
   WTP_RX_MAX_WINDOW; exactly one of d_img and d_img_next NULL; a NULL d_adv, d_slot_len or
   d_slot_len_next with window > 0; [d_slot_len, + 4*window) overlapping [d_slot_len_next,
   + 4*window); [d_img, + 1456*window) overlapping [d_img_next, + 1456*window).  Ranges that
   touch without sharing a byte are valid.

   One stream-ordered launch with no host synchronisation, no allocation, no scratch and no
   library table, so no wtp_init is needed before a capture; graph captures, replays and
   concurrent calls on different windows are independent.  wtp_last_kernel() names
   "k_rx_advance".  Fast path (16-B vectors): both images 16-B aligned (1456 = 91 * 16, so
   every slot then is); the v % 16 tail, and every other image alignment, move bytewise,
   exactly, and no access is wider than the alignment allows.  The cost follows the bytes
   that are filled, not the window: an empty slot costs the 4 + 4 bytes of its length. */
int wtp_rx_advance(const void *d_img, const uint32_t *d_slot_len, uint32_t window,
                   const uint64_t *d_adv,
                   void *d_img_next, uint32_t *d_slot_len_next, void *stream);

/* ---- multi-connection flush and slide: every flow in one pass -------------------------
   The second half of the multi-flow receive round: wtp_accept_data_packets_flows ->
   wtp_rx_build_acks_flows -> wtp_rx_deliver_flows -> wtp_rx_advance_flows, all stream-ordered,
   with the window bases moved on the device, so one captured graph serves every round of
   any number of connections with one host read at its end.  The state is accept_flows':
   flow f owns global slots [f*window, (f+1)*window) of one d_slot_len[nflows*window] and one
   image of nflows*window*1456 bytes; the limits are WTP_RX_MAX_FLOWS, WTP_RX_MAX_WINDOW and
   WTP_RX_MAX_FLOW_SLOTS.  Byte sums over the state reach 2^24 * 1456 > 2^32 and are 64-bit.

   wtp_rx_deliver_flows, stated sequentially: run_f = the number of leading slots of flow f's
   sub-window with d_slot_len <= WTP_MAX_PAYLOAD (wtp_rx_deliver's rule: WTP_SLOT_EMPTY, a
   claim pattern or any other value ends the run).  The candidates are the slots (f, s) with
   s < min(run_f, max_slots), in flow-major order (f rising, then s rising); Q_r = the 64-bit
   sum of the lengths of the candidates before rank r.  K = the largest count such that the
   first K candidates all have stream_off + Q_r + len_r <= stream_bytes: whole records only
   and a prefix of the candidate list (the predicate is monotone in r); zero-length records
   that still fit count.  k_f = the number of flow f's candidates among the first K.
   Candidate rank r < K, in slot (f, s) with length len, gives d_stream[stream_off + Q_r .. +
   len) = d_img[(f*window + s)*1456 .. + len), d_offsets_out[r] = stream_off + Q_r and
   d_lengths_out[r] = len: one packed record list, flow 0's records first, directly usable
   by wtp_crc32_batch_packed; both arrays hold nflows * min(window, max_slots) entries and
   may be NULL.  d_flow_adv[f] = k_f, always written
   for every f < nflows (64-bit: the type of wtp_rx_advance's d_adv).  d_flow_info may be
   NULL; otherwise d_flow_info[4f .. 4f+4) = {run_f, R_f, B_f, bytes_f}: R_f = the rank of the
   flow's first delivered record = the sum of k_g over g < f, B_f = the absolute stream offset
   of its first byte = stream_off + the sum of bytes_g over g < f, bytes_f = the bytes
   delivered for it; the host routes the ranges [B_f, B_f + bytes_f) of the one stream to the
   connections.  d_counts[0 .. 4) = {K, the sum of run_f, Q_K, the bytes all runs would need}
   is always written; the last value ignores max_slots and the capacity, as wtp_rx_deliver's
   P_run does.
   Consequences: with nflows == 1 every output equals wtp_rx_deliver's word for word,
   d_counts included, and d_flow_adv[0] == d_counts[0].  When everything fits, the result
   equals calling wtp_rx_deliver per flow in order with stream_off moved on by the earlier
   flows' bytes.  When it does not, the flow where the cut falls delivers a prefix and
   every later flow delivers nothing, even a record smaller than the room left: its k_f =
   0, so its window does not move and nothing is lost.
   Nothing else is written: every byte of d_stream outside [stream_off, stream_off + Q_K)
   stays as it was, the bytes that share a 16-B vector with the first and last delivered
   byte included; entries >= K of the record arrays stay as they were; d_img and d_slot_len
   are only read and no byte outside [d_img, d_img + nflows*window*1456) is loaded.
   d_stream overlapping d_img is undefined.  nflows == 0, window == 0 and max_slots == 0 are
   valid: d_counts and d_flow_adv are still written, and with max_slots == 0 the runs are
   still reported.
   d_work is the caller's scratch (any alignment, contents arbitrary on entry, unspecified on
   return; every word the call reads it has written before).  With S = nflows*window and B =
   ceil(S / 1024), wtp_rx_deliver_flows_work_bytes = 40 + 12*S + 28*B + 16*nflows (its
   arguments clamped to the limits), monotone in both arguments and at most 64 KiB + 16 bytes
   per global slot + 16 bytes per flow.
   WTP_EINVAL (before any device is touched, each with its own message): nflows >
   WTP_RX_MAX_FLOWS, window > WTP_RX_MAX_WINDOW, nflows*window (in 64 bits) >
   WTP_RX_MAX_FLOW_SLOTS; stream_off > stream_bytes; work_bytes below the size above; a NULL
   d_counts or d_work; a NULL d_flow_adv with nflows > 0; a NULL d_img or d_slot_len with
   nflows*window > 0; a NULL d_stream with nflows*window > 0 and max_slots > 0.
   Stream-ordered launches (runs, block sums, their scan, the slot scan, the per-flow
   outputs, the copy) with no host synchronisation, no allocation and no library table, so
   no wtp_init is needed before a capture; grids are sized from nflows, window and max_slots,
   never from device values, and nothing is done serially per flow: 2^20 flows of 16 slots
   and one flow of 2^20 slots are the same work.  Graph captures, replays and concurrent
   calls on different work buffers are independent.  Fast path as wtp_rx_deliver's (a 4-B
   aligned d_img; spanning, first, last and edge vectors bytewise, exactly).
   wtp_last_kernel() names "k_dflows_copy", or the last launch of the scans when nothing can
   be copied ("k_dflows_out"; "k_dflows_mid" with nflows == 0). */
size_t wtp_rx_deliver_flows_work_bytes(uint32_t nflows, uint32_t window);
int wtp_rx_deliver_flows(const void *d_img, const uint32_t *d_slot_len,
                         uint32_t nflows, uint32_t window, uint32_t max_slots,
                         void *d_stream, size_t stream_bytes, uint64_t stream_off,
                         uint64_t *d_offsets_out, uint32_t *d_lengths_out,
                         uint64_t *d_flow_adv, uint64_t *d_flow_info, uint64_t *d_counts,
                         void *d_work, size_t work_bytes, void *stream);

/* wtp_rx_advance_flows slides every flow's sub-window and base: wtp_rx_advance per flow, in
   one launch.  a_f = min(d_flow_adv[f], window), compared in 64 bits and read on the device
   when the kernel runs, so wtp_rx_deliver_flows' d_flow_adv passes as it is.  For every flow
   and every s < window, with t = s + a_f and v = d_slot_len[f*window + t] if t < window, else
   WTP_SLOT_EMPTY: d_slot_len_next[f*window + s] = v, for every v; and if v <= WTP_MAX_PAYLOAD
   and the images are given, v bytes of slot (f, t) of d_img go to slot (f, s) of d_img_next.
   Bytes [v, 1456) of a slot and slots that receive nothing stay as they were
   (wtp_rx_advance's rule, per flow).  d_seq0_next[f] = d_seq0[f] + a_f (mod 2^32): the next
   round's accept_flows reads its bases where this call left them.  d_img and d_img_next may
   both be NULL (only the lengths and bases move); d_seq0 and d_seq0_next may both be NULL
   (the bases are not moved).  The inputs are only read, nothing outside the three output
   arrays is written and no byte outside the input image is loaded.  nflows == 1 reproduces
   wtp_rx_advance.  nflows*window == 0 is valid, launches nothing and writes nothing.
   WTP_EINVAL (before any device is touched, each with its own message): a limit exceeded as
   above; exactly one of d_img and d_img_next, or of d_seq0 and d_seq0_next, NULL; a NULL
   d_flow_adv, d_slot_len or d_slot_len_next with nflows*window > 0; an output range that
   overlaps its input range: the slot_len arrays over 4*nflows*window bytes, the images over
   1456*nflows*window, seq0 over 4*nflows.  Ranges that touch are valid.
   One stream-ordered launch with no host synchronisation, allocation, scratch or library
   table, and the independence of wtp_rx_advance; wtp_last_kernel() names
   "k_rx_advance_flows".  Fast path: both images 16-B aligned; the v % 16 tail and every
   other alignment move bytewise.  The cost follows the bytes that are filled. */
int wtp_rx_advance_flows(const void *d_img, const uint32_t *d_slot_len,
                         uint32_t nflows, uint32_t window, const uint64_t *d_flow_adv,
                         const uint32_t *d_seq0,
                         void *d_img_next, uint32_t *d_slot_len_next, uint32_t *d_seq0_next,
                         void *stream);

/* wtp_tx_advance slides the sender window's state (d_acked, d_sent_ms of
   wtp_tx_ingest_acks / wtp_tx_build_retransmit) down by a entries into d_acked_next /
   d_sent_ms_next.  slots is the number of entries of each of the four arrays, the caller's
   window capacity, which may be larger than the current inflight; slots <=
   WTP_TX_MAX_INFLIGHT.  d_adv points at one device-resident uint32_t, read when the kernel
   runs: wtp_tx_ingest_acks' d_counts can be passed as it is (d_counts[0] = the advance);
   wtp_tx_build_retransmit writes its own d_counts, so a caller that runs it before the
   advance gives the two calls separate buffers.  a = min(*d_adv, slots).  For s < slots
   with t = s + a: d_acked_next[s] = d_acked[t] if t < slots, else 0, and d_sent_ms_next[s] =
   d_sent_ms[t] if t < slots, else fill_ms (any value; the entries behind the shifted ones
   belong to packets not sent yet).  With fill_ms = now_ms - timeout_ms - 1 those entries
   are due at the next wtp_tx_build_retransmit_var, which then also makes a packet's first
   transmission, in slot order with the retransmits: a sender round over records is ingest
   -> advance -> that call.  The inputs and *d_adv are only read; nothing outside
   the two output arrays is written.  slots == 0 is valid and launches nothing.  WTP_EINVAL
   (before any device is touched): slots > WTP_TX_MAX_INFLIGHT, a NULL pointer with slots >
   0, an output array overlapping an input array or the other output (arrays that touch
   are valid).  One stream-ordered launch, one lane per entry; no host synchronisation,
   allocation, scratch or library table, and the same independence of captures, replays and
   concurrent calls as wtp_rx_advance.  wtp_last_kernel() names "k_tx_advance". */
int wtp_tx_advance(const uint32_t *d_acked, const uint32_t *d_sent_ms, uint32_t slots,
                   const uint32_t *d_adv, uint32_t fill_ms,
                   uint32_t *d_acked_next, uint32_t *d_sent_ms_next, void *stream);

/* ---- the multi-connection sender: ingest, slide and rebuild every flow at once ---------
   The sender's side of the multi-flow round: wtp_tx_ingest_acks_flows -> wtp_tx_advance_flows
   -> wtp_tx_build_retransmit_var_flows, three calls whatever the number of connections, all
   stream-ordered, with the window bases moved on the device, so one captured graph serves
   every round.  Per-connection semantics are exactly those of wtp_tx_ingest_acks,
   wtp_tx_advance and wtp_tx_build_retransmit_var; only the batching across connections, and
   the bases living in device memory, are new.

   State.  All flows share one `window`.  Flow f owns global slots [f*window, (f+1)*window) of
   one d_acked[S] and one d_sent_ms[S], S = nflows*window; the global slot of (f, s) is g =
   f*window + s.  Limits: nflows <= WTP_TX_MAX_FLOWS, window <= WTP_TX_MAX_INFLIGHT and S (in
   64 bits) <= WTP_TX_MAX_FLOW_SLOTS (the one-level block ranking of the selection holds one
   count per lane of a 1024-lane block; a ring of 2^20 datagrams is already 1.5 GiB of wire).
   All flows' records sit in one table (d_base, base_bytes, d_offsets[nrec], d_lengths[nrec]),
   wtp_build_data_packets_var's layout.  Three per-flow device arrays are read when the
   kernels run, never when the call is made: d_seq0[f] = the seqNum of the flow's slot 0,
   d_rec0[f] = the table index of the record in slot 0, d_rec_end[f] = one past the flow's
   last record (constant over a transfer).  Slot (f, s) is record d_rec0[f] + s, and the
   flow's window holds inflight_f = min(window, d_rec_end[f] - d_rec0[f]) slots if d_rec_end[f]
   > d_rec0[f], else 0.  All three calls compute it the same way, so every input is defined;
   slots [inflight_f, window) of a flow are never read as window state and never counted.

   wtp_tx_ingest_acks_flows takes one batch with the ACKs of all connections in arrival
   order; d_flow[i] names the datagram's flow and any value >= nflows means "no connection".
   For every f the result is what wtp_tx_ingest_acks gives on the subsequence d_flow[i] == f,
   in index order, with seq0 = d_seq0[f], inflight = inflight_f and the flow's sub-array of
   d_acked; d_flow_adv[f] and d_flow_fresh[f] are that call's d_counts[0] (the leading ACKed
   run) and d_counts[1] (the slots that went 0 -> 1).  d_ok[i] is written for every datagram
   by wtp_tx_ingest_acks' rule, whatever its flow; d_hit[i] is the slot (selective) or a
   (cumulative) within the flow, WTP_NOT_PLACED for every datagram that does not count and
   for "no connection"; d_hit may be NULL.  In cumulative mode a flow's slots [0, the largest
   a of that flow) are filled.  d_flow_adv and d_flow_fresh are written for every f < nflows,
   also with n == 0 and for a flow no datagram names; n == 0, nflows == 0 and window == 0 are
   valid.  Nothing else in d_acked changes; every other input is only read.  nflows == 1
   reproduces wtp_tx_ingest_acks word for word.
   WTP_EINVAL (before any device is touched, each with its own message): n >= 2^31, an unknown
   mode, stride < 16, a limit exceeded, a NULL d_flow_adv or d_flow_fresh with nflows > 0, a
   NULL d_seq0, d_rec0 or d_rec_end with nflows > 0, a NULL d_acked with S > 0, a NULL
   d_dgrams, d_recv_len, d_flow or d_ok with n > 0.
   No scratch: the two per-flow arrays are the only accumulators.  Stream-ordered launches
   (selective: per-flow init, one lane per datagram, one pass over the S slots; cumulative:
   init, datagrams, the fill over the S slots, the leading run over the S slots, a per-flow
   pass), no host synchronisation, no library table, so no wtp_init is needed before a
   capture.  Nothing is serial per flow: 2^20 flows of one slot and one flow of 2^20 slots
   are the same work. */
#define WTP_TX_MAX_FLOWS      (1u << 20)
#define WTP_TX_MAX_FLOW_SLOTS (1u << 20)   /* nflows * window; equals WTP_TX_MAX_INFLIGHT */
int wtp_tx_ingest_acks_flows(const void *d_dgrams, size_t stride, const uint32_t *d_recv_len,
                             const uint32_t *d_flow, size_t n, uint32_t mode,
                             const uint32_t *d_seq0, const uint32_t *d_rec0, const uint32_t *d_rec_end,
                             uint32_t nflows, uint32_t window, uint32_t *d_acked,
                             uint8_t *d_ok, uint32_t *d_hit,
                             uint32_t *d_flow_adv, uint32_t *d_flow_fresh, void *stream);

/* wtp_tx_advance_flows slides every flow's sub-window and bases: wtp_tx_advance per flow with
   slots = window and a_f = min(d_flow_adv[f], window), read on the device when the kernel
   runs (wtp_tx_ingest_acks_flows' d_flow_adv passes as it is), in one launch with one lane per
   global slot.  For every flow and s < window with t = s + a_f: d_acked_next[f*window + s] =
   d_acked[f*window + t] if t < window, else 0, and d_sent_ms_next[f*window + s] =
   d_sent_ms[f*window + t] if t < window, else fill_ms (wtp_tx_advance's rule: with fill_ms =
   now_ms - timeout_ms - 1 the entries shifted in are due at the next build).  d_seq0_next[f] =
   d_seq0[f] + a_f and d_rec0_next[f] = d_rec0[f] + a_f, both mod 2^32: the next round's calls
   read the bases where this call left them.  d_seq0, d_rec0, d_seq0_next and d_rec0_next may
   be NULL all together; then the bases do not move.  The inputs are only read and nothing
   outside the four output arrays is written.  S == 0 is valid, launches nothing and writes
   nothing.  nflows == 1 reproduces wtp_tx_advance.
   WTP_EINVAL (before any device is touched, each with its own message): a limit exceeded;
   exactly one of d_seq0 / d_seq0_next or of d_rec0 / d_rec0_next NULL, or one pair without the
   other; with S > 0 a NULL d_flow_adv, d_acked, d_sent_ms, d_acked_next or d_sent_ms_next; an
   output range overlapping an input range or another output range: the state arrays over 4*S
   bytes, the base arrays (and d_flow_adv against the next bases) over 4*nflows bytes.  Ranges
   that touch are valid.
   One stream-ordered launch with no host synchronisation, allocation, scratch or library
   table; wtp_last_kernel() names "k_txf_advance". */
int wtp_tx_advance_flows(const uint32_t *d_acked, const uint32_t *d_sent_ms,
                         uint32_t nflows, uint32_t window, const uint32_t *d_flow_adv, uint32_t fill_ms,
                         const uint32_t *d_seq0, const uint32_t *d_rec0,
                         uint32_t *d_acked_next, uint32_t *d_sent_ms_next,
                         uint32_t *d_seq0_next, uint32_t *d_rec0_next, void *stream);

/* wtp_tx_build_retransmit_var_flows selects the due slots of every flow and builds exactly
   those datagrams into one ring.
   Selection: global slot g = (f, s) is due iff s < inflight_f, d_acked[g] == 0 and (flags &
   WTP_RETX_ALL or (uint32_t)(now_ms - d_sent_ms[g]) > timeout_ms).  Due slots are taken in
   rising g (flow 0's first, then s rising) and the first min(due, max_sel) of them are
   emitted: entry k gets d_sel[k] = g and d_sent_ms[g] = now_ms; the host routes ring entry k
   to the peer of flow d_sel[k] / window.  d_counts[0] = the number emitted, d_counts[1] = the
   number due.  The selection does not look at the records.  The cut: a ring shorter than the
   due set cuts in flow-major order, as wtp_rx_deliver_flows cuts; the flow where the cut
   falls emits a prefix of its due slots and every later flow emits nothing in this call.
   With timers the caller calls again: emitted slots are no longer due, so the next call
   takes up where this one stopped.  With WTP_RETX_ALL every call starts at flow 0 again, so
   the ring must hold the whole due set (max_sel >= S always does) or the late flows starve.
   Emit: entry k, with f = d_sel[k] / window, s = d_sel[k] - f*window and r = d_rec0[f] + s
   (mod 2^32), is valid iff r < nrec and record r satisfies wtp_build_data_packets_var's rule
   (d_lengths[r] <= WTP_MAX_PAYLOAD, d_offsets[r] <= base_bytes, d_lengths[r] <= base_bytes -
   d_offsets[r]); no entry at or above nrec of either table is read.  A valid entry writes
   d_wire[k*wire_stride ..) = htonl{type = 2, seqNum = d_seq0[f] + s (mod 2^32), length = len,
   checksum = crc32(payload)} || payload, byte-identical to oracle.build_datagram and to what
   wtp_tx_build_retransmit_var writes for that record, d_wire_len[k] = 16 + len and
   d_crc_out[k] = the checksum.  An invalid entry leaves its slot untouched, d_wire_len[k] = 0
   and d_crc_out[k] = 0.  Everything else is wtp_tx_build_retransmit_var's contract,
   unchanged: entries k >= d_counts[0], bytes [16 + len, wire_stride) of every slot and the
   timers of slots not emitted stay as they were; the record table, d_acked and the per-flow
   arrays are only read; no byte outside [d_base, d_base + base_bytes) is loaded; d_sel,
   d_wire_len and d_crc_out may be NULL; the fast path is a 16-B aligned d_wire with
   wire_stride % 16 == 0 and any source alignment, and other wire alignments are built
   bytewise, exactly.  nflows == 1 reproduces that call word for word (with its d_offsets and
   d_lengths advanced by d_rec0[0] and inflight = inflight_0).  S == 0 and max_sel == 0 are
   valid: d_counts is still written.
   Scratch: work_bytes >= wtp_tx_work_bytes(nflows*window, max_sel), the existing function and
   the existing layout, because the selection is the single-window selection over the S
   global slots with a wider predicate; the scratch contract is wtp_tx_build_retransmit's.
   WTP_EINVAL (before any device is touched, each with its own message): wire_stride < 1472; a
   limit exceeded; work_bytes too small; a NULL d_counts or d_work; with S > 0 a NULL d_base,
   d_offsets or d_lengths, a NULL d_acked or d_sent_ms, a NULL d_seq0, d_rec0 or d_rec_end; a
   NULL d_wire with S > 0 and max_sel > 0.
   Stream-ordered launches (count, select, emit) with no host synchronisation and no
   allocation; grids are sized from S and max_sel, never from device values.  The call reads
   no library table, so it needs no wtp_init before a capture; captures, replays and
   concurrent calls on different work buffers are independent.  wtp_last_kernel() names
   "k_txf_emit", or "k_txf_select" when S or max_sel is 0 and nothing can be emitted. */
int wtp_tx_build_retransmit_var_flows(const void *d_base, size_t base_bytes,
                                      const uint64_t *d_offsets, const uint32_t *d_lengths, size_t nrec,
                                      const uint32_t *d_seq0, const uint32_t *d_rec0, const uint32_t *d_rec_end,
                                      uint32_t nflows, uint32_t window,
                                      const uint32_t *d_acked, uint32_t *d_sent_ms, uint32_t now_ms,
                                      uint32_t timeout_ms, uint32_t flags,
                                      void *d_wire, size_t wire_stride, uint32_t max_sel,
                                      uint32_t *d_sel, uint32_t *d_wire_len, uint32_t *d_crc_out,
                                      uint32_t *d_counts, void *d_work, size_t work_bytes, void *stream);

/* ---- the connection table: classify by address, open and close flows -------------------
   The layer in front of and behind the multi-flow receive round.  wtp_flows_classify makes
   the round's d_flow from the datagrams' source addresses; wtp_flows_control, after
   wtp_rx_advance_flows, applies the batch's START and END datagrams (cpp/src/wReceiver.cpp:
   199-254, for one connection: ring.peer(k), open, start_seq, expected = 0): it opens flows,
   closes flows and writes the control ACKs.  The round classify -> accept_flows ->
   build_acks_flows -> deliver_flows -> advance_flows -> control is six stream-ordered calls
   for any number of connections, those that come and go included, so one captured graph
   serves every round and the host reads counters and two short event lists at its end.

   The table.  d_table is opaque, caller-owned device memory of wtp_conn_table_bytes(nbuckets)
   bytes (320 per bucket), 16-B aligned, which the caller fills with 0xFF bytes once: that
   value means "empty", d_slot_len's convention.  nbuckets is a power of two in [1,
   WTP_CONN_MAX_BUCKETS]; wtp_conn_table_bytes gives 0 for any other value.  A key is any
   WTP_CONN_KEY_BYTES = 16 bytes (a sockaddr_in as recvmmsg writes msg_name): every one of the
   2^128 values is a valid key, occupancy lives in a tag word beside the key.  A key belongs
   to exactly one bucket, wtp_conn_bucket(key16, nbuckets) (host, pure, thread-safe, touches no
   device; WTP_NO_FLOW for a NULL key or a bad nbuckets), the same function the kernels use.  A
   bucket holds WTP_CONN_WAYS live connections in any order; a lookup scans one bucket and
   nothing else (constant work, no probe chains), and freeing an entry is marking it empty
   (no tombstones).  With nbuckets >= nflows / 2 a bucket's load is Poisson with mean <= 2 and
   P(more than 16 in a bucket) is about 5.6e-11; at mean 4 it is 1.1e-6.

   wtp_flows_classify: key i is the 16 bytes at d_keys + i*key_stride.  d_flow[i] = the flow
   whose connection has that key, else WTP_NO_FLOW (every _flows call treats any value >=
   nflows as "no connection").  It only reads the table and the keys and writes d_flow[0 .. n)
   and nothing else; no byte outside [d_keys, d_keys + (n-1)*key_stride + 16) is loaded.  One
   launch, one lane per datagram.  Fast path: a 16-B aligned key is one 16-B load, a 4-B
   aligned key four dword loads; any other alignment loads bytewise.  n == 0 is valid and
   launches nothing.  WTP_EINVAL (before any device is touched, each with its own message): n
   >= 2^31; key_stride < 16; nbuckets zero, not a power of two or above the limit; a NULL
   d_keys, d_table or d_flow with n > 0; d_table not 16-B aligned.  wtp_last_kernel() names
   "k_conn_classify".

   wtp_flows_control runs at the end of the receive round, on the same stream, with the same
   batch (ring, d_recv_len, d_keys), accept's d_ok, classify's d_flow (a snapshot of the table
   as it was on entry to the round; with any other d_flow the result is unspecified, though
   no access leaves the caller's arrays) and the d_seq0 and d_slot_len that the advance
   wrote, the next round's state.  d_recv_len is not read: d_ok says that the header is there.
   Per-flow arrays: d_flow_start[nflows], the START seqNum of the flow's connection,
   meaningful only while the flow is open; d_seq0[nflows] and d_slot_len[nflows*window],
   accept_flows' state.  The free-id ring is d_free[nflows] and d_free_pos[2] = {head, count},
   a FIFO: the caller initialises d_free[j] = j, head = 0, count = nflows; opens take ids from
   the head, closes append at (head + count) mod nflows.  Popped and pushed cells are disjoint
   by construction, so no launch reads and writes one cell.  The cells hold ids below nflows; one
   that does not is never used as a flow (the open it would have served is refused), and that
   call's d_counts and d_free_pos are unspecified.

   Datagram i is a control datagram iff d_ok[i] != 0 and its type is START or END
   (wtp_tx_ingest_acks' treatment of ACKs; stricter than the reference, which does not check
   them).  Everything else gets the verdict WTP_CTL_NONE.  Stated sequentially: all STARTs are
   processed in index (arrival) order, then all ENDs in index order; each is judged by f =
   d_flow[i], the entry snapshot.
   START, f < nflows (the key already has a connection): seqNum == d_flow_start[f] gives
   WTP_CTL_START_DUP, answered (the START's ACK was lost), no state changes; otherwise
   WTP_CTL_START_OTHER, dropped (opt/Receiver.cpp:148-150).
   START, f >= nflows (a new key): the first such datagram of a key needs a free entry in its
   bucket, else WTP_CTL_REFUSED_BUCKET, and then a free id, else WTP_CTL_REFUSED_FULL.  Neither
   refusal is answered and neither changes state (an entry taken during the attempt is
   released): the sender's START times out and comes again.  Otherwise WTP_CTL_OPENED,
   answered: with g = the id at the ring's head, the table maps the key to g, d_flow_start[g] =
   seqNum, d_seq0[g] = 0 (the endpoints' expected = 0) and d_slot_len[g*window .. +window) =
   WTP_SLOT_EMPTY.  A later datagram with the same new key in the same batch is judged
   against what the first one did: START_DUP or START_OTHER by its seqNum if the first
   opened, the first's refusal verdict otherwise.  Flow ids are therefore deterministic: the
   r-th connection opened in arrival order gets the r-th id of the ring.  With nflows == 0
   the table is not looked at and every START is REFUSED_FULL.
   END, f >= nflows: WTP_CTL_END_STALE, answered (the duplicate END of a connection already
   closed, wReceiver.cpp:219-221, or an END with no connection).  f < nflows and seqNum !=
   d_flow_start[f]: WTP_CTL_END_OTHER, dropped.  f < nflows, seqNum equal, window > 0 and
   d_slot_len[f*window] != WTP_SLOT_EMPTY: WTP_CTL_END_BUSY, dropped (the flow still holds
   undelivered data, the stream cut fell before it; the sender's END comes again; only slot 0
   is looked at).  Otherwise the first such datagram of flow f is WTP_CTL_CLOSED, answered:
   the key's entry is freed and f is appended to the ring; the flow's window is not touched
   (the next open resets it).  Later such ENDs of f in the batch are END_STALE, answered.  A
   flow opened in this call cannot be closed in it (its datagrams carry WTP_NO_FLOW), so opens
   and closes are independent within a call, and an entry or an id freed in a call serves no
   open of that call.

   Determinism and overflow.  The result is exactly the sequential statement's whenever no
   bucket overflows in the call: live entries plus distinct new keys hashing to the bucket
   exceed WTP_CONN_WAYS.  On overflow: the number opened into the bucket is exactly its free
   entries, further limited by the free ids, in arrival order among the keys that hold an
   entry; the remaining keys are refused and nothing of theirs is left in the table;
   everything outside that bucket's new keys is exact.  Which keys of the bucket are refused,
   and REFUSED_BUCKET against REFUSED_FULL when both are short, is unspecified.

   Outputs.  The answered datagrams are ranked in arrival order across both kinds; rank k <
   max_acks becomes d_ack_wire[k*ack_stride .. +16) = htonl{3, the datagram's own seqNum, 0, 0}
   and d_ack_src[k] = i: one 16-B store where the slot is 16-B aligned, bytes otherwise.  State
   changes are applied whether or not the ACK fits: a peer whose ACK was cut retransmits and
   gets START_DUP or END_STALE.  d_opened[r], d_opened_src[r] = the flow and the datagram index
   of the r-th open, d_closed[q] = the q-th closed flow, in arrival order; each list has at
   most nflows entries.  d_verdict[i] = the WTP_CTL_* code.  d_ack_src, d_opened_src and
   d_verdict may be NULL.  d_counts[0 .. 6) = {ACKs emitted, ACKs eligible, opened, closed,
   datagrams refused full, datagrams refused bucket}, always written, also for n == 0, nflows
   == 0 and max_acks == 0, which are all valid.  d_free_pos = {head + opened mod nflows, count
   - opened + closed}.  Nothing else is written: entries past the counts and bytes [16,
   ack_stride) of a slot stay as they were; d_seq0, d_flow_start and d_slot_len of flows not
   opened stay as they were; ring cells neither popped nor pushed stay as they were; every
   input is only read.  While the call runs a table tag may hold a claim (0x80000000 |
   datagram index, d_slot_len's encoding); a completed call leaves none behind.

   d_work is the caller's scratch (any alignment, contents arbitrary on entry, unspecified on
   return; every word the call reads it has written before).  wtp_conn_scratch_bytes(n, nflows)
   = 20 + 4*n + 12*ceil(n / 1024) + 8*nflows (its arguments clamped to the limits), monotone in
   both arguments and at most 64 KiB + 8 bytes per datagram + 8 bytes per flow.
   WTP_EINVAL (before any device is touched, each with its own message): n >= 2^31; stride <
   16; key_stride < 16; ack_stride < 16; a bad nbuckets; nflows > WTP_RX_MAX_FLOWS, window >
   WTP_RX_MAX_WINDOW, nflows*window > WTP_RX_MAX_FLOW_SLOTS; work_bytes too small; a NULL
   d_counts or d_work; a NULL d_table, d_flow_start, d_seq0, d_free, d_free_pos, d_opened or
   d_closed with nflows > 0; a NULL d_slot_len with nflows*window > 0; a NULL d_dgrams,
   d_recv_len, d_ok, d_keys or d_flow with n > 0; a NULL d_ack_wire with n > 0 and max_acks >
   0; d_table not 16-B aligned.
   Stream-ordered launches (mark and claim, count, open, close, emit, reset) with no host
   synchronisation, no allocation and no library table, so no wtp_init is needed before a
   capture; grids are sized from n, nflows and window, never from device values, and nothing
   is serial per datagram or per flow: a batch of 64 Ki STARTs is the same kind of work as
   one START.  Graph captures, replays and concurrent calls on different tables, states and
   work buffers are independent.  wtp_last_kernel() names "k_conn_reset", or "k_conn_emit"
   when n == 0 or nflows*window == 0 and no slot can be reset. */
#define WTP_NO_FLOW          0xFFFFFFFFu
#define WTP_CONN_KEY_BYTES   16u
#define WTP_CONN_WAYS        16u
#define WTP_CONN_MAX_BUCKETS (1u << 20)
#define WTP_CTL_NONE           0u
#define WTP_CTL_OPENED         1u
#define WTP_CTL_START_DUP      2u
#define WTP_CTL_START_OTHER    3u
#define WTP_CTL_REFUSED_FULL   4u
#define WTP_CTL_REFUSED_BUCKET 5u
#define WTP_CTL_CLOSED         6u
#define WTP_CTL_END_STALE      7u
#define WTP_CTL_END_OTHER      8u
#define WTP_CTL_END_BUSY       9u
size_t wtp_conn_table_bytes(uint32_t nbuckets);
uint32_t wtp_conn_bucket(const void *key16, uint32_t nbuckets);
int wtp_flows_classify(const void *d_keys, size_t key_stride, size_t n,
                       const void *d_table, uint32_t nbuckets,
                       uint32_t *d_flow, void *stream);
size_t wtp_conn_scratch_bytes(size_t n, uint32_t nflows);
int wtp_flows_control(const void *d_dgrams, size_t stride, const uint32_t *d_recv_len,
                      const void *d_keys, size_t key_stride, const uint32_t *d_flow,
                      const uint8_t *d_ok, size_t n,
                      void *d_table, uint32_t nbuckets, uint32_t nflows, uint32_t window,
                      uint32_t *d_flow_start, uint32_t *d_seq0, uint32_t *d_slot_len,
                      uint32_t *d_free, uint32_t *d_free_pos,
                      void *d_ack_wire, size_t ack_stride, uint32_t max_acks, uint32_t *d_ack_src,
                      uint32_t *d_opened, uint32_t *d_opened_src, uint32_t *d_closed,
                      uint32_t *d_verdict, uint32_t *d_counts,
                      void *d_work, size_t work_bytes, void *stream);

/* ---- the running whole-file CRC-32 of every connection --------------------------------
   wtp_rx_digest_flows keeps, per flow, the CRC-32 and the byte count of everything delivered
   for the flow so far, in caller-owned device memory: what wtp_crc32_buffer gives for one
   transfer, for any number of connections in a fixed number of launches.  It is the seventh
   call of the receive round, classify -> accept_flows -> build_acks_flows -> deliver_flows ->
   advance_flows -> control -> digest, on the same stream and in the same captured graph.

   Inputs and state.  d_stream[0 .. stream_bytes) is wtp_rx_deliver_flows' stream and
   d_flow_info its output, passed as it is: d_flow_info[4f+2] = B_f, the absolute stream offset
   of the flow's first delivered byte, and d_flow_info[4f+3] = bytes_f; words 4f+0 and 4f+1 are
   not read.  All values are read on the device when the kernels run.  The state is
   d_flow_crc[nflows] and d_flow_bytes[nflows], caller-owned, updated in place; zero means
   "nothing yet" (the CRC of the empty message is 0), so the caller zeroes both once.

   The fold, stated sequentially for every f < nflows.  The range is valid iff B_f <=
   stream_bytes and bytes_f <= stream_bytes - B_f (wtp_build_data_packets_var's rule, in 64
   bits, no overflow).  A valid flow with bytes_f > 0: d_flow_crc[f] = combine(d_flow_crc[f],
   crc32(d_stream[B_f .. B_f + bytes_f)), bytes_f), zlib semantics, bit-identical to
   wtp_crc32_combine, and d_flow_bytes[f] += bytes_f (mod 2^64).  A valid flow with bytes_f ==
   0 and an invalid flow leave both words as they were; the invalid one is counted and no
   status flag is set (as in wtp_tx_ingest_acks).  The ranges of different flows may overlap
   and come in any order: each flow is folded on its own, so every input is defined.  No byte
   outside [d_stream, d_stream + stream_bytes) is loaded, the aligned 16-B vector loads
   included: a vector that crosses an edge of the buffer is loaded bytewise, as in the builder.

   Report, then reset, both after the fold and in this order.  Report: for q < min(
   *d_report_count, max_report) with g = d_report[q]: d_report_crc[q] = d_flow_crc[g] and
   d_report_bytes[q] = d_flow_bytes[g]; g >= nflows writes 0 and 0xFFFFFFFFFFFFFFFF.  Entries
   past the count stay as they were.  Reset: for j < min(*d_reset_count, max_reset) with g =
   d_reset[j] < nflows: d_flow_crc[g] = 0 and d_flow_bytes[g] = 0; duplicates and ids >= nflows
   are harmless.  A flow in both lists is reported with its folded value and then zeroed.
   Either list may be absent: both of its pointers NULL.  The intended wiring, after
   wtp_flows_control on the same stream: d_report = d_closed and d_report_count = control's
   d_counts + 3; d_reset = d_opened and d_reset_count = control's d_counts + 2.  That is exact:
   control refuses to close a flow whose slot 0 is still filled (WTP_CTL_END_BUSY), so at the
   end of the round in which a flow closes everything of its file has been delivered and
   folded; and an id freed in a call serves no open of that call, so an id that is reused is
   zeroed at the end of the round that opened it, before the next round delivers its first
   data.  A caller without a connection table calls this right after deliver with both lists
   NULL.

   d_counts[0 .. 4) (64-bit) = {bytes folded, flows folded, ranges refused, reports written},
   always written, also for nflows == 0, which is valid.  Nothing else is written: d_stream and
   every other input are only read, and the memory behind every output array is untouched.
   Consequence: with nflows == 1, a zeroed state and any sequence of rounds, d_flow_crc[0]
   equals wtp_crc32_buffer over the concatenation of everything delivered.

   d_work is the caller's scratch (any alignment, contents arbitrary on entry, unspecified on
   return; every word the call reads it has written before).  wtp_rx_digest_scratch_bytes(
   nflows) = 16432 + 12*nflows (its argument clamped to WTP_RX_MAX_FLOWS), monotone and at most
   64 KiB + 16 bytes per flow.
   WTP_EINVAL (before any device is touched, each with its own message): nflows >
   WTP_RX_MAX_FLOWS; work_bytes below the size above; a NULL d_counts or d_work; with nflows >
   0 a NULL d_flow_info, d_flow_crc or d_flow_bytes, or a NULL d_stream with stream_bytes > 0;
   exactly one of d_reset and d_reset_count NULL; exactly one of d_report and d_report_count
   NULL; a report list with max_report > 0 and a NULL d_report_crc or d_report_bytes.
   Stream-ordered launches (unit counts, their scan, the hash, the merge of its records, the
   fold, the report, the reset) with no host synchronisation, no allocation and no library
   table: the hash uses its unit's own compile-time tables, so no wtp_init is needed before a
   capture.  Grids are sized from nflows, stream_bytes and the list capacities (the hash runs
   on a capped persistent grid), never from device values, and the number of launches does
   not depend on nflows.  Nothing is serial per flow: the delivered ranges are cut into 4-KiB
   units that spread over the grid flow-major, so 2^20 flows of one short record, 2^16 flows
   that are mostly empty and one flow of 2^20 slots are the same kind of work, and the atomic
   updates of one flow's word stay below the waves of one workgroup whatever its size.  Graph
   captures, replays and concurrent calls on different states and work buffers are
   independent.  Fast path: every 16-B vector inside the buffer, at any byte phase of d_stream
   and of B_f.  wtp_last_kernel() names "k_dig_reset", or "k_dig_report" when no reset list is
   given, max_reset == 0 or nflows == 0. */
size_t wtp_rx_digest_scratch_bytes(uint32_t nflows);
int wtp_rx_digest_flows(const void *d_stream, size_t stream_bytes,
                        const uint64_t *d_flow_info, uint32_t nflows,
                        uint32_t *d_flow_crc, uint64_t *d_flow_bytes,
                        const uint32_t *d_reset, const uint32_t *d_reset_count, uint32_t max_reset,
                        const uint32_t *d_report, const uint32_t *d_report_count, uint32_t max_report,
                        uint32_t *d_report_crc, uint64_t *d_report_bytes,
                        uint64_t *d_counts, void *d_work, size_t work_bytes, void *stream);

/* ---- whole-buffer CRC: the fold of payload CRCs ------------------------------------
   The reference's crc32(buf, size) takes any size; these give it for device-resident data
   of any size from the per-chunk CRCs, by zlib's crc32_combine identity
   crc32(A || B) = crc32(A) * x^(8|B|) mod P ^ crc32(B).

   Host: crc32(A || B) from crc32(A), crc32(B) and |B|.  Square and multiply,
   O(log len_b); any uint64 len_b (x has order dividing 2^32 - 1, so len_b acts mod
   2^32 - 1).  combine(c, 0, 0) == c and combine(0, c, len) == c, so a fold over chunks
   starts from 0.  Thread-safe, touches no device. */
uint32_t wtp_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);

/* Device: *d_out = CRC-32 of the concatenation of n payloads, in index order, from their
   CRCs d_crc[0 .. n) (e.g. the checksums in the builder's headers, or d_crc_out of the
   verify call) and their lengths; the payloads themselves are never read, so no
   WTP_MAX_KERNEL_LEN limit and no status flag apply.  d_len != NULL: payload i has
   d_len[i] bytes, any uint32 value (0 included).  d_len == NULL: payloads 0 .. n-2 have
   `len` bytes and payload n-1 has `last_len` (the builder's chunking: len = 1456,
   last_len = total - (n-1)*1456), any uint64 values.  n == 0 writes 0, the CRC of the
   empty message (unlike the batch calls, and like *d_ack above, the one result is
   always written).  d_out is one uint32_t and nothing beside it is written; d_crc and
   d_len are only read.  d_work is the caller's scratch of at least
   wtp_crc32_concat_work_bytes(n) bytes (<= 64 KiB for any n), 4-byte aligned: its
   contents on entry are arbitrary (it need not be zeroed), on return unspecified.
   work_bytes below that size, or a NULL d_work, d_out, or d_crc with n > 0, returns
   WTP_EINVAL.  One or two stream-ordered launches, no host synchronisation, no
   allocation, no state kept: graph captures on any stream, replays of one graph and
   concurrent calls on different work buffers are independent.  wtp_last_kernel() names
   "k_concat_fold" (d_len == NULL) or "k_concat_var". */
size_t wtp_crc32_concat_work_bytes(size_t n);
int wtp_crc32_concat(const uint32_t *d_crc, const uint32_t *d_len, uint64_t len, uint64_t last_len,
                     size_t n, void *d_work, size_t work_bytes, uint32_t *d_out, void *stream);

/* Device: *d_out = crc32(d_buf[0 .. nbytes)) for any nbytes (64-bit) and any base
   alignment; nbytes == 0 writes 0.  The 16-B aligned interior runs through the braided
   kernel of wtp_crc32_batch_fixed in 1456-B chunks (their CRCs go to d_work), the head
   before the first 16-B boundary (<= 15 B) and the tail (< 1456 B) are hashed by two
   extra workgroups of the fold, so a misaligned base costs no more than those.  d_buf is
   only read.  d_work, work_bytes, d_out, launches and independence as for
   wtp_crc32_concat, with wtp_crc32_buffer_work_bytes(nbytes) = the concat size + 4 bytes
   per 1456-B chunk; the braided launch plus two more.  Call wtp_init before capturing. */
size_t wtp_crc32_buffer_work_bytes(size_t nbytes);
int wtp_crc32_buffer(const void *d_buf, size_t nbytes, void *d_work, size_t work_bytes,
                     uint32_t *d_out, void *stream);

/* ---- host-memory wrappers (library-owned pinned staging, synchronous) -------------- */

/* Host memory: *h_crc = crc32(h_buf[0 .. nbytes)), 0 for nbytes == 0.  The chunk CRCs of
   wtp_crc32_host_chunked (chunk = 1456) folded on the host with one constant-multiplier
   operator, four table lookups per chunk. */
int wtp_crc32_host_buffer(const void *h_buf, size_t nbytes, uint32_t *h_crc);

/* Like wtp_crc32_batch_fixed but payloads and results live in host memory. */
int wtp_crc32_host_batch_fixed(const void *h_payloads, size_t stride, size_t len, size_t n,
                               uint32_t *h_out);

/* The wSender path (cpp/src/base/Sender.cpp:82-92): CRC of every `chunk`-byte chunk of
   a host buffer (last chunk may be short).  Pipelined: pinned H2D -> CRC -> D2H,
   double-buffered on two HIP streams.  h_out needs ceil(nbytes/chunk) entries. */
int wtp_crc32_host_chunked(const void *h_buf, size_t nbytes, size_t chunk, uint32_t *h_out);

/* wtp_crc32_host_chunked over several GPUs of this process: the chunks split into ndev
   contiguous ranges, one pinned pipeline (and PCIe link, and staging thread) per device,
   results written straight into h_out (chunks are independent, Crc32.hpp:92-96: no
   collective).  devices = NULL means devices 0 .. ndev-1; ndev <= 0 means every
   visible device.  The calling thread's current device is unchanged on return. */
int wtp_crc32_host_chunked_multi(const void *h_buf, size_t nbytes, size_t chunk, uint32_t *h_out,
                                 const int *devices, int ndev);

/* The wReceiver path, host buffers: same semantics as wtp_crc32_verify_batch.  When the
   ring and recv_len both live in page-locked memory (wtp_host_alloc) and the ring is at
   most 4 MiB, the kernel reads them in place (one launch + one sync per call); other
   batches go through the library's pinned double-buffered copy pipeline.
   WTP_HOST_ZEROCOPY=0 in the environment forces the pipeline. */
int wtp_crc32_host_verify(const void *h_dgrams, size_t stride, const uint32_t *h_recv_len,
                          size_t n, uint8_t *h_ok, uint32_t *h_crc_out);

/* The fused builder from and to host memory (wSender --crc gpu): same layout as
   wtp_build_data_packets; the bytes of a wire slot past its datagram are unspecified.
   Pinned (wtp_host_alloc) payloads and wire buffers move by DMA directly, others through
   the library's pinned slabs; synchronous. */
int wtp_host_build_data_packets(const void *h_payloads, size_t total_bytes, uint32_t seq0,
                                void *h_wire, size_t wire_stride, uint32_t *h_wire_len);

/* Pinned (page-locked) host allocation for zero-copy staging, e.g. wSender reads its
   input file straight into such a buffer.  NULL on failure. */
void *wtp_host_alloc(size_t bytes);
void wtp_host_free(void *p);

/* ---- synthetic inputs (bench / tests) ------------------------------
   d_out[i] = byte (start_byte+i) of the splitmix64 stream for `seed`:
   byte g = (mix64(seed + ((g>>3)+1)*0x9E3779B97F4A7C15) >> (8*(g&7))) & 0xFF. */
int wtp_synth_fill(void *d_out, uint64_t start_byte, size_t nbytes, uint64_t seed, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* WTP_CRC32_H */
