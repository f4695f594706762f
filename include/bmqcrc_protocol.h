/* bmqcrc_protocol.h -- the batch callers of the CRC32C path (libbmqcrc.so).
 *
 * BlazingMQ computes or checks one CRC32C per message in four loops.  Each
 * entry point here walks the reference's own wire/disk format on the host
 * ("scan": CPU only, no GPU needed), then CRCs every message with ONE batched
 * MI355X call (bmqcrc_crc32c_batch / bmqcrc_crc32c_verify, include/bmqcrc.h).
 * Paths are relative to /root/reference.
 *
 *   bmqcrc_put_event_fill_crcs  bmqp::PutEventBuilder::packMessage CRC
 *                               (src/groups/bmq/bmqp/bmqp_puteventbuilder.cpp:302,320,400,413;
 *                               written to PutHeader::d_crc32c, bmqp_protocol.h:1497)
 *   bmqcrc_put_event_verify     bmqp::PutMessageIterator recompute
 *                               (bmqp_putmessageiterator.cpp:670-679)
 *   bmqcrc_recover_verify       mqbs::FileStore::recoverMessages CRC check
 *                               (src/groups/mqb/mqbs/mqbs_filestore.cpp:2495-2624)
 *   bmqcrc_csl_validate         mqbc::ClusterStateLedgerUtil::validateLog
 *                               (src/groups/mqb/mqbc/mqbc_clusterstateledgerutil.cpp:248-336)
 *
 * Buffers are host memory (an mmap'd file or an event blob flattened into one
 * buffer).  Scans return the number of messages found (which may exceed
 * `cap`; only `cap` entries are written, so cap = 0 sizes the arrays) or a
 * negative BMQCRC_E* code with bmqcrc_last_error() naming the offending
 * offset.  GPU entry points return BMQCRC_ENODEV without a gfx950 device;
 * the C++ spellings at the end of this header fall back to the host CRC.
 */
#ifndef BMQCRC_PROTOCOL_H
#define BMQCRC_PROTOCOL_H

#include <stdint.h>

#include "bmqcrc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- PUT events (bmqp_protocol.h:746 EventHeader, :1374 PutHeader) ------ */

/* Walk a PUT event: EventHeader (length must equal `len`, type e_PUT = 2)
 * then PutHeader-framed messages.  For message i: app_off/app_len = its
 * application data (after header and options, before the 1..4 padding
 * bytes) and crc_pos = byte offset of its big-endian PutHeader CRC field. */
int64_t bmqcrc_put_event_scan(const void* event, uint64_t len, uint64_t* app_off,
                              uint32_t* app_len, uint64_t* crc_pos, uint64_t cap);

/* Deferred CRC: CRC every message's application data in one batch and write
 * each result big-endian into its PutHeader.  Returns the message count. */
int64_t bmqcrc_put_event_fill_crcs(void* event, uint64_t len, const bmqcrc_opts* opts);

/* Check every PutHeader CRC against its application data in one batch.
 * *n_msgs = messages, *n_bad = mismatches, bad_idx = up to bad_cap message
 * indices in ascending order. */
int bmqcrc_put_event_verify(const void* event, uint64_t len, uint64_t* n_msgs, uint64_t* n_bad,
                            uint64_t* bad_idx, uint64_t bad_cap, const bmqcrc_opts* opts);

/* ABI 2.10.  Pack device-resident payloads into PUT events, on the device:
 * what PutEventBuilder::packMessage does per message on the host (header,
 * append, CRC, padding; bmqp_puteventbuilder.cpp:80-173, 302-320), for n
 * messages in one call.  Message i's application data (properties + payload)
 * is the lengths[i] bytes at src + src_offsets[i].
 *
 * Wire format: per event an 8-byte EventHeader (BE length, (1 << 6) | 2,
 * header words 2, two zero bytes); per message a 36-byte PutHeader
 * (flags << 28 | messageWords; optionsWords 0 | CAT 0 | headerWords 9; BE
 * queue id; GUID; BE CRC32-C at +28; four zero bytes), the application data,
 * and pad = 4 - len % 4 bytes each equal to pad.  Options, compression (CAT)
 * and schema ids are out of scope for this version: those fields are zero.
 *
 * Layout: with B[i] = 36 + lengths[i] + pad(lengths[i]), P its 64-bit
 * exclusive prefix and e(i) the event of message i, the events lie back to
 * back in dst: message i's header at 8 (e(i) + 1) + P[i], event e at
 * 8 e + P[event_first[e]].  Bytes of dst at or beyond the total are never
 * written.  A message of length 0 is legal (four padding bytes, CRC 0).
 *
 * Options.  Device pointers only: BMQCRC_F_DEVICE_PTRS is required,
 *   BMQCRC_F_ASYNC allowed; any other flag, ndevices > 1, a null required
 *   array, dst not 4-byte aligned, [dst, dst + dst_bytes) meeting
 *   [src, src + src_bytes), max_event_bytes above (2^28 - 1) * 4, event_first
 *   == NULL with n_events != 1, or n_events outside [1, n] is BMQCRC_EINVAL,
 *   answered on the host before the device lookup.
 * All or nothing, decided on the device (all sums in 64 bits): every
 *   src_offsets[i] + lengths[i] <= src_bytes; event_first[0] == 0, strictly
 *   increasing, last entry == n; every event's length <= max_event_bytes;
 *   the total <= dst_bytes; and the payload within the copy kernel's
 *   2^32 - 1 16-byte pieces (counted as len / 16 rounded up, plus one, per
 *   non-empty message).  On any violation nothing is written to dst, out or
 *   event_offsets; a synchronous call returns BMQCRC_EINVAL naming the kind
 *   and the lowest offending message (SRC_RANGE) or event index, and after
 *   an asynchronous call bmqcrc_last_put_pack reports them.  Of several
 *   violations the lowest kind is reported.
 * *total_bytes (may be NULL) is written by a synchronous call only: the
 *   bytes of all events, 0 when refused.
 * State.  As bmqcrc_crc32c_copy: takes the workspace mutex of (device,
 *   stream); leaves the shape prediction and every bmqcrc_last_* record of
 *   the batch and copy calls as they were; restores the caller's current
 *   device; allocates its own workspace on first use and when n grows (12
 *   bytes per message, 16 without `out`), which bmqcrc_reserve does not
 *   cover; is not meant to be captured into a hipGraph; is deterministic.
 *   n == 0 writes nothing and reports 0 messages, 0 events, 0 bytes. */
#define BMQCRC_PUT_PACK_OK 0
#define BMQCRC_PUT_PACK_SRC_RANGE 1       /* index: the lowest message outside src */
#define BMQCRC_PUT_PACK_EVENT_FIRST 2     /* index: the lowest bad entry (n_events: the last) */
#define BMQCRC_PUT_PACK_EVENT_TOO_BIG 3   /* index: the lowest event above max_event_bytes */
#define BMQCRC_PUT_PACK_DST_TOO_SMALL 4   /* index: the lowest event ending past dst_bytes */
#define BMQCRC_PUT_PACK_TOO_MANY_PIECES 5 /* index 0: beyond the copy kernel's piece limit */

typedef struct bmqcrc_put_pack {
    uint32_t struct_size;          /* sizeof(bmqcrc_put_pack) */
    uint32_t reserved;             /* 0 */
    const void* src;               /* device: payload arena */
    uint64_t src_bytes;
    const uint64_t* src_offsets;   /* device, n */
    const uint32_t* lengths;       /* device, n: application-data bytes (properties + payload) */
    const int32_t* queue_ids;      /* device, n */
    const uint8_t* guids;          /* device, 16 n */
    const uint8_t* flags;          /* device, n, low 4 bits used; NULL = 0 */
    const uint64_t* event_first;   /* device, n_events + 1: event e holds messages
                                      [event_first[e], event_first[e+1]); NULL = one event
                                      (n_events must then be 1) */
    uint64_t n;
    uint64_t n_events;
    uint64_t max_event_bytes;      /* 0 = PutHeader::k_MAX_SIZE_SOFT (66 MiB); at most
                                      (2^28-1)*4 so MessageWords cannot overflow */
    void* dst;                     /* device, 4-byte aligned: events laid back to back */
    uint64_t dst_bytes;
    uint64_t* event_offsets;       /* device, n_events + 1, may be NULL: byte offset of each
                                      event in dst; the last entry is the total */
    uint32_t* out;                 /* device, n, may be NULL: the CRCs (host order) */
} bmqcrc_put_pack;

int bmqcrc_put_event_pack(const bmqcrc_put_pack* p, uint64_t* total_bytes, const bmqcrc_opts* opts);

/* ABI 2.10.  Result of the previous bmqcrc_put_event_pack on (device,
 * stream); waits for it.  *n_msgs and *n_events = its n and n_events,
 * *total_bytes = the bytes of all events (0 when refused), *refused_kind =
 * BMQCRC_PUT_PACK_OK or the kind refused and *refused_index its index.  All
 * zero before the first pack there.  Any pointer may be NULL. */
int bmqcrc_last_put_pack(int device, void* stream, uint64_t* n_msgs, uint64_t* n_events,
                         uint64_t* total_bytes, uint32_t* refused_kind, uint64_t* refused_index);

/* ABI 2.11.  Pack device-resident payloads into DATA-file records and their
 * journal MessageRecords, on the device: what FileStore::writeMessageRecord
 * does per accepted message on the host (mqbs_filestore.cpp:5634-5747:
 * DataHeader, payload, dword padding, then the journal record pointing at
 * it), for n messages in one call.  Message i's application data is the
 * lengths[i] bytes at src + src_offsets[i].
 *
 * DATA records (dst).  R[i] = 12 + lengths[i] + pad with pad = 8 - (12 +
 *   lengths[i]) % 8, that is 1..8 bytes each equal to pad; Q = the 64-bit
 *   exclusive prefix of R.  Record i lies at dst + Q[i]: a 12-byte DataHeader
 *   (mqbs_filestoreprotocol.h:703) of three big-endian words, (3 << 29) |
 *   R[i] / 4; optionsWords 0 | flags (data_flags[i], else 0); schema id 0;
 *   then the application data and the padding.  Bytes of dst at or beyond
 *   Q[n] are never written.  A length of 0 is legal (12 + 4 padding bytes,
 *   CRC 0).  Options, compression (CAT) and schema ids are out of scope for
 *   this version: those fields are zero.
 * Journal records (journal_dst).  Record i occupies [60 i, 60 i + 60), a
 *   MessageRecord (:1125) as writeMessageRecord fills it: @0 BE u16 (1 << 12)
 *   | (refcount & 0xFFF); @2 the 6-byte BE sequence number first_seq + i; @8
 *   BE lease_id; @12 BE u64 timestamps[i], else `timestamp`; @20 refcount >>
 *   12 (refcount = the low 20 bits of ref_counts[i], else 1); @21 0 (CAT);
 *   @22 queue_keys[5 i ..]; @27 file_key; @32 BE u32 MessageOffsetDwords =
 *   (data_file_pos + Q[i]) / 8; @36 guids[16 i ..]; @52 the BE stored CRC;
 *   @56 the magic 0x2A724563.
 * CRC and verify on write.  out[i] (may be NULL) always receives the CRC32-C
 *   computed from the bytes copied, seed 0.  Without `expected` that is the
 *   stored CRC.  With `expected` (device, n, host order) the stored CRC is
 *   expected[i] -- the broker stores the value that arrived in the PutHeader,
 *   so a corrupt payload stays detectable at recovery -- and the call counts
 *   the messages with out[i] != expected[i] (n_bad) and reports the lowest
 *   (first_bad; n when none).  Mismatches do not fail the call.
 * record_offsets (may be NULL): device, n + 1, receives Q; the last entry is
 *   the total.
 *
 * Options.  Device pointers only: BMQCRC_F_DEVICE_PTRS is required,
 *   BMQCRC_F_ASYNC allowed; any other flag, ndevices > 1, a wrong struct_size
 *   or reserved, a null required array, dst not 8-byte or journal_dst not
 *   4-byte aligned, data_file_pos zero or no multiple of 8 (recovery treats
 *   offset 0 as invalid), lease_id 0, first_seq 0 or first_seq + n - 1 above
 *   2^48 - 1, 60 n > journal_bytes, or any two of [src, +src_bytes), [dst,
 *   +dst_bytes), [journal_dst, +journal_bytes) meeting is BMQCRC_EINVAL,
 *   answered on the host before the device lookup.
 * All or nothing, decided on the device (all sums in 64 bits): every R[i] / 4
 *   within the DataHeader's 29 bits; every src_offsets[i] + lengths[i] <=
 *   src_bytes; Q[n] <= dst_bytes; data_file_pos + Q[n] <= 8 (2^32 - 1), where
 *   MessageOffsetDwords stops; and the payload within the copy kernel's
 *   2^32 - 1 16-byte pieces (counted as len / 16 rounded up, plus one, per
 *   non-empty message).  On any violation nothing is written to dst,
 *   journal_dst, out or record_offsets; a synchronous call returns
 *   BMQCRC_EINVAL naming the kind and the lowest offending message, and after
 *   an asynchronous call bmqcrc_last_records_pack reports them.  Of several
 *   violations the lowest kind is reported.
 * *result (may be NULL) is written by a synchronous call only.
 * State.  As bmqcrc_put_event_pack: takes the workspace mutex of (device,
 *   stream); leaves the shape prediction and every bmqcrc_last_* record of
 *   the batch, copy and PUT-pack calls as they were; restores the caller's
 *   current device; allocates its own workspace on first use and when n grows
 *   (12 bytes per message, 16 without `out`), which bmqcrc_reserve does not
 *   cover; is not meant to be captured into a hipGraph; is deterministic.
 *   n == 0 writes nothing and reports zeros. */
#define BMQCRC_REC_PACK_OK 0
#define BMQCRC_REC_PACK_RECORD_TOO_BIG 1  /* index: the lowest message with R/4 > 2^29-1 */
#define BMQCRC_REC_PACK_SRC_RANGE 2       /* index: the lowest message outside src */
#define BMQCRC_REC_PACK_DST_TOO_SMALL 3   /* index: the lowest message ending past dst_bytes */
#define BMQCRC_REC_PACK_DATA_FILE_FULL 4  /* index: the lowest message ending past 8 (2^32-1) */
#define BMQCRC_REC_PACK_TOO_MANY_PIECES 5 /* index 0: beyond the copy kernel's piece limit */

typedef struct bmqcrc_records_pack {
    uint32_t struct_size;          /* sizeof(bmqcrc_records_pack) */
    uint32_t reserved;             /* 0 */
    const void* src;               /* device: payload arena */
    uint64_t src_bytes;
    const uint64_t* src_offsets;   /* device, n */
    const uint32_t* lengths;       /* device, n: application-data bytes */
    const uint8_t* queue_keys;     /* device, 5 n */
    const uint8_t* guids;          /* device, 16 n */
    const uint8_t* data_flags;     /* device, n: DataHeader flags; NULL = 0 */
    const uint32_t* ref_counts;    /* device, n, low 20 bits used; NULL = 1 */
    const uint64_t* timestamps;    /* device, n; NULL = `timestamp` for all */
    const uint32_t* expected;      /* device, n, host order: the CRCs to store and to check
                                      against; NULL = store the computed ones */
    uint8_t file_key[5];           /* the DATA file's key, into every record */
    uint8_t reserved2[3];          /* ignored */
    uint32_t lease_id;             /* primary lease id, not 0 */
    uint64_t first_seq;            /* sequence number of message 0, not 0 */
    uint64_t timestamp;
    uint64_t data_file_pos;        /* byte position in the DATA file that dst stands for:
                                      a multiple of 8, not 0 */
    uint64_t n;
    void* dst;                     /* device, 8-byte aligned: DATA records back to back */
    uint64_t dst_bytes;
    void* journal_dst;             /* device, 4-byte aligned: 60-byte records back to back */
    uint64_t journal_bytes;        /* at least 60 n */
    uint64_t* record_offsets;      /* device, n + 1, may be NULL: Q, the total last */
    uint32_t* out;                 /* device, n, may be NULL: the computed CRCs (host order) */
} bmqcrc_records_pack;

/* All fields zero before the first call on (device, stream). */
typedef struct bmqcrc_records_result {
    uint64_t n_msgs;
    uint64_t data_bytes;           /* Q[n]; 0 when refused */
    uint64_t journal_bytes;        /* 60 n; 0 when refused */
    uint64_t n_bad;                /* messages whose computed CRC differs from expected[] */
    uint64_t first_bad;            /* the lowest of them; n_msgs when none */
    uint32_t refused_kind;         /* BMQCRC_REC_PACK_OK or the kind refused */
    uint32_t reserved;             /* 0 */
    uint64_t refused_index;
} bmqcrc_records_result;

int bmqcrc_message_records_pack(const bmqcrc_records_pack* p, bmqcrc_records_result* result,
                                const bmqcrc_opts* opts);

/* ABI 2.11.  Result of the previous bmqcrc_message_records_pack on (device,
 * stream); waits for it.  `result` may be NULL. */
int bmqcrc_last_records_pack(int device, void* stream, bmqcrc_records_result* result);

/* ABI 2.12.  The inverse of bmqcrc_put_event_pack: PUT events in device
 * memory are walked ON THE DEVICE, and every message's descriptors come back
 * as the arrays the packers take.  It is PutMessageIterator::next with its
 * recompute (bmqp_putmessageiterator.cpp:670-679) for a batch of events in
 * one asynchronous call: with `out` every PutHeader CRC is checked against
 * its application data.  No payload byte and no descriptor crosses PCIe.
 *
 * Events.  Event e is bytes [event_offsets[e], event_offsets[e + 1]) of
 *   `events`; event_offsets == NULL means one event, the whole buffer.
 * Messages are numbered event by event in walk order; event_first (may be
 *   NULL) receives the exclusive prefix of the per-event counts, n_msgs last.
 *   Message i yields app_offsets[i] (byte offset in `events` of its
 *   application data), lengths[i], queue_ids[i], guids[16 i ..], flags[i] (the
 *   PutHeader's 4 flag bits) and expected[i] (the PutHeader CRC, host order):
 *   exactly what bmqcrc_put_event_scan reports for the event, with the
 *   event's offset added to positions.
 * What it accepts.  Message options, the compression type (CAT) and schema
 *   ids are not interpreted, but events that carry them are accepted: PutHeader
 *   headerWords may be 8..31, optionsWords is skipped as the host walk skips
 *   it, an EventHeader longer than 8 bytes is honoured, and an event of 8
 *   bytes with no message is legal.
 * Options.  Device pointers only: BMQCRC_F_DEVICE_PTRS is required,
 *   BMQCRC_F_ASYNC allowed; any other flag, ndevices > 1, a wrong struct_size
 *   or reserved, `events`, app_offsets or lengths null, `events` not 4-byte
 *   aligned, event_offsets == NULL with n_events != 1, n_events or msg_cap at
 *   or above 2^32, or any given output array meeting [events, events +
 *   events_bytes) is BMQCRC_EINVAL, answered on the host before the device
 *   lookup.  n_events == 0 writes nothing and reports zeros.
 * All or nothing, decided on the device.  One violation anywhere refuses the
 *   call, and a refused call writes nothing to any output array.  Within an
 *   event the violation reported is the first in walk order: the checks of
 *   bmqcrc_put_event_scan in its order, refused_offset being the event's
 *   offset plus the offset its error text names.  Across events the lowest
 *   kind wins and within it the lowest event.  For EVENT_OFFSETS
 *   refused_offset is event_offsets[refused_event], for TOO_MANY_MESSAGES the
 *   event's start.  A synchronous call returns BMQCRC_EINVAL naming kind,
 *   event and offset; after an asynchronous call bmqcrc_last_put_unpack
 *   reports them.  The walk never loads a byte it has not first shown to lie
 *   inside its event, and event_offsets is checked against events_bytes
 *   before any event byte is read.
 * CRC pass.  With out != NULL the application data of every message is CRC'd
 *   (seed 0) by the batch kernels, planned, on the call's own stream; n_bad
 *   and first_bad count the messages whose out[i] differs from the PutHeader
 *   CRC.  Mismatches do not fail the call.  The call never synchronises under
 *   BMQCRC_F_ASYNC and the device alone knows n_msgs, so the pass always runs
 *   over msg_cap slots (the unused ones are empty messages): a tight msg_cap
 *   is the caller's job.  The pass reads its descriptors from the call's own
 *   workspace, never from the caller's arrays.
 * After a successful call entries [n_msgs, msg_cap) of app_offsets, lengths,
 *   expected and out are unspecified and the other arrays untouched there;
 *   nothing at or beyond msg_cap is ever written.
 * *result (may be NULL) is written by a synchronous call only.
 * State.  Takes the workspace mutex of (device, stream); restores the
 *   caller's current device; allocates its own workspace on first use and
 *   when msg_cap or n_events grows (20 bytes per slot of msg_cap, 16 per
 *   event), which bmqcrc_reserve does not cover; is not meant to be captured
 *   into a hipGraph; is deterministic.  With out != NULL it counts as a
 *   BMQCRC_F_DEVICE_PTRS | BMQCRC_F_PLAN batch of msg_cap messages for
 *   bmqcrc_last_launch, bmqcrc_last_plan, bmqcrc_last_offsets and the shape
 *   prediction; with out == NULL those stay untouched.  The records of
 *   bmqcrc_last_copy, bmqcrc_last_put_pack and bmqcrc_last_records_pack are
 *   never touched. */
#define BMQCRC_PUT_UNPACK_OK 0
#define BMQCRC_PUT_UNPACK_EVENT_OFFSETS 1     /* event_offsets[e] > event_offsets[e+1], event_offsets[e+1] >
                                                 events_bytes, or event_offsets[e] not a multiple of 4 */
#define BMQCRC_PUT_UNPACK_EVENT_HEADER 2      /* shorter than 8; length field != event size; type != PUT;
                                                 headerWords * 4 outside [8, size] */
#define BMQCRC_PUT_UNPACK_PUT_HEADER 3        /* truncated PutHeader; headerWords * 4 < 32; messageWords 0,
                                                 past the event, or <= header + options */
#define BMQCRC_PUT_UNPACK_PADDING 4           /* last byte of the message not in 1..4 or larger than the data */
#define BMQCRC_PUT_UNPACK_TOO_MANY_MESSAGES 5 /* more than msg_cap messages; index: the lowest event whose
                                                 last message does not fit */

typedef struct bmqcrc_put_unpack {
    uint32_t struct_size, reserved;       /* sizeof, 0 */
    const void* events;                   /* device, 4-byte aligned */
    uint64_t events_bytes;
    const uint64_t* event_offsets;        /* device, n_events + 1: event e is [event_offsets[e], event_offsets[e+1]);
                                             NULL = one event, the whole buffer (n_events must be 1) */
    uint64_t n_events;
    uint64_t msg_cap;                     /* capacity of the per-message arrays, < 2^32 */
    uint64_t* app_offsets;                /* device, msg_cap: byte offset in `events` of the application data */
    uint32_t* lengths;                    /* device, msg_cap */
    int32_t* queue_ids;                   /* device, msg_cap, may be NULL */
    uint8_t* guids;                       /* device, 16 msg_cap, may be NULL */
    uint8_t* flags;                       /* device, msg_cap, may be NULL: PutHeader flags (4 bits) */
    uint32_t* expected;                   /* device, msg_cap, may be NULL: the PutHeader CRCs, host order */
    uint32_t* out;                        /* device, msg_cap, may be NULL: the computed CRCs; NULL = walk only */
    uint64_t* event_first;                /* device, n_events + 1, may be NULL: first message of each event, n last */
} bmqcrc_put_unpack;

/* All fields zero before the first call on (device, stream). */
typedef struct bmqcrc_put_unpack_result {
    uint64_t n_events, n_msgs;            /* n_msgs 0 when refused */
    uint64_t n_bad, first_bad;            /* header CRC != computed CRC; first_bad = n_msgs when none */
    uint32_t refused_kind, reserved;
    uint64_t refused_event, refused_offset; /* offset: byte in `events` that the host walk would name */
} bmqcrc_put_unpack_result;

int bmqcrc_put_event_unpack(const bmqcrc_put_unpack* p, bmqcrc_put_unpack_result* result,
                            const bmqcrc_opts* opts);

/* ABI 2.12.  Result of the previous bmqcrc_put_event_unpack on (device,
 * stream); waits for it.  `result` may be NULL. */
int bmqcrc_last_put_unpack(int device, void* stream, bmqcrc_put_unpack_result* result);

/* ABI 2.13.  The inverse of bmqcrc_message_records_pack: a run of journal
 * records and a window of the DATA file in device memory are walked ON THE
 * DEVICE, every MessageRecord and its DataHeader checked as
 * FileStore::recoverMessages checks them (mqbs_filestore.cpp:2390-2575), and
 * every message's descriptors come back as the arrays the packers take.  With
 * `out` every stored CRC is checked against its application data in the same
 * asynchronous call.  No payload byte and no descriptor crosses PCIe.
 *
 * Records.  Record r is bytes [60 r, 60 r + 60) of `journal`: the caller
 *   passes the record run, not the journal file with its headers (the packer's
 *   journal_dst is such a run; bmqcrc_journal_bounds bounds a file's).  `data`
 *   stands for bytes [data_file_pos, data_file_pos + data_bytes) of the DATA
 *   file; data_file_pos 0 means the whole file from its first byte.  The
 *   packer's dst and data_file_pos go straight in.
 * Messages are the MESSAGE records (type 1) with select[r] != 0 (select ==
 *   NULL: all of them), numbered in ascending record order.  Message k yields
 *   record_index[k]; app_offsets[k], the byte offset IN `data` of its
 *   application data (usable as src_offsets with src = data in both packers);
 *   lengths[k]; queue_keys[5 k ..] (record bytes @22); guids[16 k ..] (@36);
 *   data_flags[k] (the DataHeader's flags byte); ref_counts[k] (20 bits: byte
 *   @20 << 12, or'ed with the low 12 bits of the BE u16 @0); timestamps[k] (BE
 *   u64 @12); expected[k] (the stored CRC @52, host order): the inputs of
 *   bmqcrc_message_records_pack, so that unpack followed by pack with the same
 *   file_key, lease_id, first_seq and data_file_pos reproduces both byte
 *   streams.  DataHeader options are skipped, not interpreted: the
 *   application data starts at o - data_file_pos + 4 headerWords + 4
 *   optionsWords.
 * Options.  Device pointers only: BMQCRC_F_DEVICE_PTRS is required,
 *   BMQCRC_F_ASYNC allowed; any other flag, ndevices > 1, a wrong struct_size
 *   or reserved, `journal`, `data`, app_offsets or lengths null, `journal` not
 *   4-byte or `data` not 8-byte aligned, data_file_pos no multiple of 8,
 *   n_records or msg_cap at or above 2^32, 60 n_records > journal_bytes, or
 *   any given output array meeting [journal, journal + journal_bytes) or
 *   [data, data + data_bytes) is BMQCRC_EINVAL, answered on the host before
 *   the device lookup.  n_records == 0 writes nothing and reports zeros.
 * All or nothing, decided on the device.  One violation anywhere refuses the
 *   call, and a refused call writes nothing to any output array.  A record is
 *   checked in the host walk's order (walk_recovery, bmqcrc_journal_scan) and
 *   raises its first violation; across records the lowest kind wins and
 *   within it the lowest record.  With o = 8 MessageOffsetDwords and end =
 *   data_bytes, a selected MESSAGE record's DATA record is malformed when
 *   o - data_file_pos + 8 > end; headerWords or messageWords is 0; 4
 *   (headerWords + optionsWords) >= 4 messageWords; the record ends past end;
 *   or its last byte, the padding count, is not in 1..8 or exceeds what the
 *   header and the options leave.  Record types 2..15 are validated under
 *   RECORD_HEADER and then skipped, as the host walk skips them.  A MESSAGE
 *   record with select[r] == 0 is checked up to DATA_OFFSET, takes no slot and
 *   is counted in n_skipped: no byte of its DATA record is read (where the
 *   host walk says `continue` for deleted and purged messages).  A
 *   synchronous call returns BMQCRC_EINVAL naming kind and record; after an
 *   asynchronous call bmqcrc_last_records_unpack reports them.
 * Not restated here, the caller's business: the primary sequence number
 *   (lease id, sequence number) ordering checks, queue liveness
 *   (BMQCRC_RECOVERY_INVALID_QUEUE_KEY), the selection itself (DELETION and
 *   PURGE bookkeeping: `select` carries its outcome), and the journal bounds
 *   (the caller passes a bounded run).  bmqcrc_journal_select (ABI 2.14,
 *   below) makes the first three on the device and yields `select`.
 * CRC pass.  With out != NULL the application data of every message is CRC'd
 *   (seed 0) by the batch kernels, planned, on the call's own stream; n_bad
 *   and first_bad count the slots whose out[k] differs from expected[k].
 *   Mismatches do not fail the call.  The call never synchronises under
 *   BMQCRC_F_ASYNC and the device alone knows n_msgs, so the pass always runs
 *   over msg_cap slots (the unused ones are empty messages): a tight msg_cap
 *   is the caller's job.  The pass reads its descriptors from the call's own
 *   workspace, never from the caller's arrays.
 * After a successful call entries [n_msgs, msg_cap) of app_offsets, lengths,
 *   expected and out are unspecified and the other arrays untouched there;
 *   nothing at or beyond msg_cap is ever written.
 * *result (may be NULL) is written by a synchronous call only.
 * State.  As bmqcrc_put_event_unpack: takes the workspace mutex of (device,
 *   stream); restores the caller's current device; allocates its own
 *   workspace on first use and when msg_cap or n_records grows (20 bytes per
 *   slot of msg_cap, 17 per record), which bmqcrc_reserve does not cover; is
 *   not meant to be captured into a hipGraph; is deterministic.  With out !=
 *   NULL it counts as a BMQCRC_F_DEVICE_PTRS | BMQCRC_F_PLAN batch of msg_cap
 *   messages for bmqcrc_last_launch, bmqcrc_last_plan, bmqcrc_last_offsets and
 *   the shape prediction; with out == NULL those stay untouched.  The records
 *   of bmqcrc_last_copy, bmqcrc_last_put_pack, bmqcrc_last_records_pack and
 *   bmqcrc_last_put_unpack are never touched. */
#define BMQCRC_REC_UNPACK_OK 0
#define BMQCRC_REC_UNPACK_RECORD_HEADER 1     /* any record: type 0, lease id 0, sequence number 0, or the
                                                 magic @56 != 0x2A724563 */
#define BMQCRC_REC_UNPACK_MESSAGE_RECORD 2    /* MESSAGE record with an all-zero GUID or queue key
                                                 (recovery rc -16) */
#define BMQCRC_REC_UNPACK_DATA_OFFSET 3       /* MESSAGE record: o is 0, below data_file_pos or above
                                                 data_file_pos + data_bytes (rc -11) */
#define BMQCRC_REC_UNPACK_DATA_RECORD 4       /* selected MESSAGE record with a malformed DATA record (rc -17) */
#define BMQCRC_REC_UNPACK_TOO_MANY_MESSAGES 5 /* more selected MESSAGE records than msg_cap; index: the
                                                 record that would take slot msg_cap */

typedef struct bmqcrc_records_unpack {
    uint32_t struct_size, reserved;       /* sizeof, 0 */
    const void* journal;                  /* device, 4-byte aligned: 60-byte records back to back */
    uint64_t journal_bytes;               /* at least 60 n_records */
    uint64_t n_records;                   /* < 2^32 */
    const void* data;                     /* device, 8-byte aligned: the DATA-file window */
    uint64_t data_bytes;
    uint64_t data_file_pos;               /* byte position in the DATA file that data[0] stands for:
                                             a multiple of 8 */
    const uint8_t* select;                /* device, n_records, may be NULL: 0 = leave this MESSAGE record out */
    uint64_t msg_cap;                     /* capacity of the per-message arrays, < 2^32 */
    uint32_t* record_index;               /* device, msg_cap, may be NULL: the journal record of each slot */
    uint64_t* app_offsets;                /* device, msg_cap: byte offset in `data` of the application data */
    uint32_t* lengths;                    /* device, msg_cap */
    uint8_t* queue_keys;                  /* device, 5 msg_cap, may be NULL */
    uint8_t* guids;                       /* device, 16 msg_cap, may be NULL */
    uint8_t* data_flags;                  /* device, msg_cap, may be NULL: DataHeader flags */
    uint32_t* ref_counts;                 /* device, msg_cap, may be NULL: 20 bits */
    uint64_t* timestamps;                 /* device, msg_cap, may be NULL */
    uint32_t* expected;                   /* device, msg_cap, may be NULL: the stored CRCs, host order */
    uint32_t* out;                        /* device, msg_cap, may be NULL: the computed CRCs; NULL = walk only */
} bmqcrc_records_unpack;

/* All fields zero before the first call on (device, stream). */
typedef struct bmqcrc_records_unpack_result {
    uint64_t n_records;
    uint64_t n_msgs, n_skipped;           /* slots taken; unselected MESSAGE records; both 0 when refused */
    uint64_t n_bad, first_bad;            /* stored CRC != computed CRC; first_bad: a slot, n_msgs when none */
    uint32_t refused_kind, reserved;
    uint64_t refused_index;               /* a record index */
} bmqcrc_records_unpack_result;

int bmqcrc_message_records_unpack(const bmqcrc_records_unpack* p,
                                  bmqcrc_records_unpack_result* result, const bmqcrc_opts* opts);

/* ABI 2.13.  Result of the previous bmqcrc_message_records_unpack on (device,
 * stream); waits for it.  `result` may be NULL. */
int bmqcrc_last_records_unpack(int device, void* stream, bmqcrc_records_unpack_result* result);

/* ---- partition recovery (mqbs_filestoreprotocol.h:306,426,483,703,953-1990) */

/* mqbs::FileStore::recoverMessages result codes (mqbs_filestore.cpp:1073-1091)
 * that the record selection below can produce. */
#define BMQCRC_RECOVERY_SUCCESS 0
#define BMQCRC_RECOVERY_INVALID_PRIMARY_LEASE_ID (-2)
#define BMQCRC_RECOVERY_INVALID_SEQ_NUMBER (-3)
#define BMQCRC_RECOVERY_INVALID_QUEUE_OP_RECORD (-4)
#define BMQCRC_RECOVERY_NULL_QUEUE_KEY (-5)
#define BMQCRC_RECOVERY_DUPLICATE_QUEUE_KEY (-7)
#define BMQCRC_RECOVERY_INVALID_QUEUE_KEY (-8)
#define BMQCRC_RECOVERY_INVALID_DATA_OFFSET (-11)
#define BMQCRC_RECOVERY_INVALID_SYNC_PT_SUB_TYPE (-12)
#define BMQCRC_RECOVERY_INVALID_DELETION_RECORD (-14)
#define BMQCRC_RECOVERY_INVALID_CONFIRM_RECORD (-15)
#define BMQCRC_RECOVERY_INVALID_MESSAGE_RECORD (-16)
#define BMQCRC_RECOVERY_INVALID_DATA_RECORD (-17)

/* The queues recoverMessages knows (its `withCSL` argument and
 * `queueKeyInfoMap`).  cfg == NULL or with_csl == 0: the live queues are the
 * keys of the journal's own QueueOp CREATION records (the reference's first
 * pass).  with_csl != 0: the cluster state's live queues, n_queue_keys
 * 5-byte mqbu::StorageKey values at queue_keys. */
typedef struct bmqcrc_recovery_cfg {
    uint32_t struct_size; /* sizeof(bmqcrc_recovery_cfg) */
    int32_t with_csl;
    const uint8_t* queue_keys;
    uint64_t n_queue_keys;
} bmqcrc_recovery_cfg;

/* The MESSAGE records whose payload FileStore::recoverMessages CRCs
 * (mqbs_filestore.cpp:2603-2624), selected exactly as it does: the journal
 * is bounded by its last sync point and last valid record
 * (mqbs_filestoreprotocolutil.cpp:165-289) and walked backwards twice; a
 * MESSAGE record is skipped when its GUID has a later DELETION record, its
 * queue a later whole-queue PURGE, or it precedes its queue's last
 * QueueOp DELETION -- and for skipped records the DATA file is not read.
 * Records come out in that backward order: record_off = journal offset,
 * app_off / app_len = application data of its DATA record (DataHeader +
 * options + app data + 1..8 padding bytes), crc = the stored CRC32C.
 * *recovery_rc = the reference's result (0 or BMQCRC_RECOVERY_*) and
 * *error_record_off the offending record's offset when it is not 0; the
 * records before that point are still returned (the reference had CRC'd
 * them).  Any output array may be NULL.  CPU only. */
int64_t bmqcrc_journal_scan(const void* journal, uint64_t jlen, const void* data, uint64_t dlen,
                            const bmqcrc_recovery_cfg* cfg, int* recovery_rc,
                            uint64_t* error_record_off, uint64_t* record_off, uint64_t* app_off,
                            uint32_t* app_len, uint32_t* crc, uint64_t cap);

/* The journal's bounds as JournalFileIterator computes them: *last_sync_point
 * = offset of the last well-formed SYNCPOINT record, *last_record_off = the
 * last valid record after it (0 = none; mqbs_filestoreprotocolutil.cpp:165-289).
 * Records past *last_record_off (a torn write, a pre-allocated zero tail)
 * are not part of the journal.  CPU only. */
int bmqcrc_journal_bounds(const void* journal, uint64_t jlen, uint64_t* last_sync_point,
                          uint64_t* last_record_off);

/* Recovery CRC check of a whole partition: the selection of
 * bmqcrc_journal_scan, then one batched verify on the GPU.  *n_msgs = records
 * CRC'd; mismatches are what the reference raises as a RECOVERY alarm and
 * keeps going (mqbs_filestore.cpp:2613-2624): *n_bad of them, the first
 * min(*n_bad, bad_cap) in the order the reference raises them (backward
 * journal order) in bad_record_off.  *recovery_rc / *error_record_off as
 * in bmqcrc_journal_scan. */
int bmqcrc_recover_verify(const void* journal, uint64_t jlen, const void* data, uint64_t dlen,
                          const bmqcrc_recovery_cfg* cfg, int* recovery_rc,
                          uint64_t* error_record_off, uint64_t* n_msgs, uint64_t* n_bad,
                          uint64_t* bad_record_off, uint64_t bad_cap, const bmqcrc_opts* opts);

/* ABI 2.14.  The selection of bmqcrc_journal_scan for a run of journal records
 * that lies in HBM: which MESSAGE records FileStore::recoverMessages CRCs, as
 * the `select` bytes bmqcrc_message_records_unpack takes, with the reference's
 * result code and the offending record -- the two backward passes of
 * walk_recovery restated as order-free reductions, so
 * no record is walked on the host.  Device pointers only, one device:
 * BMQCRC_F_DEVICE_PTRS is required and BMQCRC_F_ASYNC allowed; every other
 * flag, unknown flag bits, ndevices > 1, a wrong struct_size, a non-zero
 * reserved field, a null journal or select, a null queue_keys with
 * n_queue_keys > 0, a misaligned journal, journal_bytes != 60 n_records,
 * n_records >= 2^32 and queue_cap == 0 are BMQCRC_EINVAL before the device
 * lookup.  n_records == 0 succeeds with an empty result.
 * The run.  Record r is journal[60 r .. 60 r + 60); the host calls name a
 *   record by its file offset, first record's offset + 60 r.  The caller bounds
 *   the top: the last record is the journal's last valid record, as
 *   bmqcrc_journal_bounds gives it for a file (bmqcrc_message_records_pack and
 *   a replica know their count).  The walk covers the records above the
 *   highest one with type 0, lease id 0, sequence number 0 or a wrong magic;
 *   that record and those below it are not in the journal: select = 0 there
 *   and no failure.
 * What is decided.  The same recovery_rc, offending record and selected set as
 *   bmqcrc_journal_scan, given the same with_csl / queue_keys, with ONE stated
 *   exception: no DATA byte is read (data_file_bytes only bounds the two
 *   DATA-offset checks: a MESSAGE record's 8 x MessageOffsetDwords being 0 or
 *   above the file, and a sync point's data offset).  So
 *   BMQCRC_RECOVERY_INVALID_DATA_RECORD (-17) is never raised here: a selected
 *   message whose DATA record is malformed stays selected, and
 *   bmqcrc_message_records_unpack then refuses it under
 *   BMQCRC_REC_UNPACK_DATA_RECORD.  The INVALID_QUEUE_KEY check of a MESSAGE
 *   record, which the reference makes after the DATA checks, is made as if
 *   those had passed.
 * Result.  A first-pass failure (QueueOp records) selects nothing:
 *   first_record == n_records.  Otherwise, with E the highest failing record
 *   of the second pass, select[r] = 0 for r <= max(E, the walk's lower end)
 *   and first_record is the record above that; the three counts cover
 *   [first_record, n_records) only.  A non-zero recovery_rc is a result, not
 *   an error: the call returns BMQCRC_OK.  More distinct queue keys (QueueOp
 *   records' and queue_keys') than queue_cap is the refusal
 *   BMQCRC_JSEL_TOO_MANY_QUEUES: select is all zero, first_record ==
 *   n_records, and a synchronous call returns BMQCRC_EINVAL naming queue_cap.
 * *result (may be NULL) is written by a synchronous call only; after an
 *   asynchronous one bmqcrc_last_journal_select waits and reports.
 * State.  As bmqcrc_message_records_unpack: takes the workspace mutex of
 *   (device, stream); restores the caller's current device; allocates its own
 *   workspace on first use and when n_records or queue_cap grows (25 to 33
 *   bytes per record and 48 to 96 per queue key it can hold), which
 *   bmqcrc_reserve does not cover; is not meant to be captured into a hipGraph; is deterministic.  The
 *   shape prediction and the records of every other bmqcrc_last_* call are
 *   never touched. */
#define BMQCRC_JSEL_OK 0
#define BMQCRC_JSEL_TOO_MANY_QUEUES 1   /* more distinct queue keys than queue_cap */

typedef struct bmqcrc_journal_select_args {
    uint32_t struct_size, reserved;       /* sizeof, 0 */
    const void* journal;                  /* device, 4-byte aligned: n_records 60-byte records, the record run */
    uint64_t journal_bytes;               /* == 60 * n_records */
    uint64_t n_records;                   /* < 2^32 */
    uint64_t data_file_bytes;             /* size of the DATA file: the DATA-offset checks only; no DATA byte is read */
    int32_t with_csl, reserved2;
    const uint8_t* queue_keys;            /* device, 5 * n_queue_keys bytes; with_csl only, may be NULL when 0 keys */
    uint64_t n_queue_keys;
    uint64_t queue_cap;                   /* most distinct queue keys (QueueOp records' plus queue_keys') the call holds */
    uint8_t* select;                      /* device, n_records, out */
} bmqcrc_journal_select_args;

/* All fields zero before the first call on (device, stream). */
typedef struct bmqcrc_journal_select_result {
    uint64_t n_records;
    uint64_t first_record;                /* select[] is meaningful on [first_record, n_records), 0 below */
    uint64_t n_selected, n_deleted, n_purged;  /* MESSAGE records of that run: kept; skipped by a DELETION
                                                  GUID; skipped by a queue PURGE or queue DELETION */
    uint64_t error_record;                /* record index; n_records when recovery_rc == 0 */
    int32_t recovery_rc;                  /* 0 or BMQCRC_RECOVERY_* */
    uint32_t refused_kind;                /* BMQCRC_JSEL_* */
} bmqcrc_journal_select_result;

int bmqcrc_journal_select(const bmqcrc_journal_select_args* p, bmqcrc_journal_select_result* result,
                          const bmqcrc_opts* opts);

/* ABI 2.14.  Result of the previous bmqcrc_journal_select on (device, stream);
 * waits for it.  `result` may be NULL. */
int bmqcrc_last_journal_select(int device, void* stream, bmqcrc_journal_select_result* result);

/* ABI 2.15.  The replica's side of replication: STORAGE events in device
 * memory are applied ON THE DEVICE to a run of the journal file and a window of
 * the DATA file, also in device memory -- FileStore::processStorageEvent with
 * FileStoreUtil::writeMessageRecordImpl for a batch of events in one
 * asynchronous call, and with what the reference leaves to recovery: the
 * application data of every DATA message is moved by the fused copy of
 * bmqcrc_crc32c_copy, whose CRC32-C is compared with the one the producer
 * stored.  No payload byte and no descriptor crosses PCIe.
 *
 * Events.  Event e is bytes [event_offsets[e], event_offsets[e + 1]) of
 *   `events`; event_offsets == NULL means one event, the whole buffer.  An
 *   event is an EventHeader of type STORAGE (8) or PARTITION_SYNC (10) and
 *   storage messages back to back: a StorageHeader of headerWords * 4 >= 12
 *   bytes, a 60-byte journal record and, for the types DATA (1) and QLIST (2),
 *   a payload: messageWords counts all three.  A DATA message's payload is its
 *   whole DATA record: DataHeader, options, application data, 1..8 padding
 *   bytes.  An event of 8 bytes with no message is legal.
 * Messages are numbered event by event in walk order, i = 0 .. n_msgs - 1;
 *   event_first (may be NULL) receives the exclusive prefix of the per-event
 *   counts, n_msgs last.
 * The replica's state.  partition_id; journal_pos and data_file_pos, the byte
 *   positions in the journal and the DATA file that journal_dst[0] and
 *   data_dst[0] stand for; (lease_id, seq), the write head: the primary
 *   sequence number of the last record applied, lease_id 0 when none is known
 *   yet (seq must be 0 then).
 * What is written, byte for byte what the reference's replica appends to its
 *   two files: journal_dst + 60 i receives message i's journal record,
 *   whatever its type.  With R[i] = 4 x DataHeader.messageWords for a DATA
 *   message, 0 for any other, and Q the 64-bit exclusive prefix of R, a DATA
 *   message's record goes to data_dst + Q[i]: DataHeader, option words and
 *   padding bytes copied as they are, the application data moved by the fused
 *   copy.  A QLIST message's payload is written nowhere (the QLIST file stays
 *   on the host): payload_offsets / payload_lengths report it.
 * Per-message outputs, each of msg_cap entries and each may be NULL:
 *   types[i] (StorageMessageType), flags[i] (the StorageHeader's 5 flag bits,
 *   bit 0 RECEIPT_REQUESTED), payload_offsets[i] / payload_lengths[i] (what
 *   follows the journal record: byte offset in `events`, bytes),
 *   record_offsets[i] = Q[i] with Q[n_msgs] behind the last (msg_cap + 1
 *   entries), lengths[i] (application data bytes), expected[i] (the
 *   MessageRecord's CRC at byte 52, host order), out[i] (the computed CRC);
 *   the last three are 0 for a message that is not DATA.
 * Verify on write.  n_bad counts the DATA messages whose computed CRC differs
 *   from the stored one, first_bad is the lowest (n_msgs when none).
 *   Mismatches do not fail the call and the bytes are applied all the same:
 *   whether to withhold the receipt is the caller's decision.
 * Options.  Device pointers only: BMQCRC_F_DEVICE_PTRS is required,
 *   BMQCRC_F_ASYNC allowed; any other flag, ndevices > 1, a wrong struct_size
 *   or reserved; `events`, journal_dst or data_dst null; `events` or
 *   journal_dst not 4-byte aligned, data_dst not 8-byte aligned;
 *   event_offsets == NULL with n_events != 1; n_events or msg_cap at or above
 *   2^32; journal_pos 0 or no multiple of 4; data_file_pos 0 or no multiple of
 *   8; partition_id above 65535; lease_id == 0 with seq != 0; any destination
 *   or output array meeting [events, events + events_bytes) or a destination
 *   is BMQCRC_EINVAL, answered on the host before the device lookup.
 *   n_events == 0 writes nothing and reports zeros with the write head
 *   unchanged.
 * All or nothing, decided on the device.  One violation anywhere refuses the
 *   call, and a refused call writes nothing to journal_dst, data_dst or any
 *   output array.  Across events the lowest kind wins and within it the lowest
 *   event (kinds 1..5) or message (kinds 6..8); within an event the violation
 *   reported is the first in walk order.  The walk never loads a byte it has
 *   not first shown to lie inside its event.  refused_event, refused_index and
 *   refused_offset name the event, the message and a byte of `events`:
 *   EVENT_OFFSETS    event_offsets[e] (the offset), the event's first message;
 *   EVENT_HEADER     the event's offset plus 0 (shorter than 8, or the length
 *                    field), 4 (the type) or 5 (headerWords); its first message;
 *   STORAGE_HEADER   the StorageHeader's offset and its message;
 *   DATA_RECORD      the DataHeader's offset and its message;
 *   TOO_MANY_MESSAGES the event's start and first message;
 *   OUT_OF_SYNC, DST_TOO_SMALL  the message, its event, its StorageHeader's
 *                    offset; TOO_MANY_PIECES names message 0.
 *   A message's number counts, in every event before it, the messages in front
 *   of that event's first violation (all of them in a well-formed event).
 *   OUT_OF_SYNC and the kinds behind it are evaluated only when the walk
 *   (kinds 1..5) refused nothing.  The reference answers an event that is out
 *   of sync by ignoring it or by aborting the broker; here it is a refusal.  A
 *   synchronous call returns BMQCRC_EINVAL naming kind, event, message and
 *   offset; after an asynchronous call bmqcrc_last_storage_apply reports them.
 * Stricter than the reference.  DATA_RECORD applies the conditions of
 *   BMQCRC_REC_UNPACK_DATA_RECORD, with "the record ends past end" read as
 *   "past the message"; the reference only asks that the record fit the blob.
 *   Nothing StorageEventBuilder emits is refused.  Bytes of a DATA message
 *   beyond 60 + R are ignored.
 * The copy runs over all msg_cap slots (the unused ones are empty messages):
 *   a tight msg_cap is the caller's job.  After a successful call entries
 *   [n_msgs, msg_cap) of the output arrays are untouched, and nothing at or
 *   beyond msg_cap (msg_cap + 1 for record_offsets) is ever written.
 * *result (may be NULL) is written by a synchronous call only.
 * State.  As bmqcrc_message_records_unpack: takes the workspace mutex of
 *   (device, stream); restores the caller's current device; allocates its own
 *   workspace on first use and when msg_cap or n_events grows (56 bytes per
 *   slot of msg_cap, 16 per event), which bmqcrc_reserve does not cover; is
 *   not meant to be captured into a hipGraph; is deterministic.  The copy's
 *   counters live in the call's own scratch: the shape prediction and the
 *   records of every other bmqcrc_last_* call are never touched. */
#define BMQCRC_STORAGE_APPLY_OK 0
#define BMQCRC_STORAGE_APPLY_EVENT_OFFSETS 1     /* event_offsets[e] > event_offsets[e+1], event_offsets[e+1] >
                                                    events_bytes, or event_offsets[e] not a multiple of 4 */
#define BMQCRC_STORAGE_APPLY_EVENT_HEADER 2      /* shorter than 8; length field != event size; type neither
                                                    STORAGE nor PARTITION_SYNC; headerWords * 4 outside [8, size] */
#define BMQCRC_STORAGE_APPLY_STORAGE_HEADER 3    /* fewer than 12 bytes left; headerWords * 4 < 12; messageWords * 4
                                                    below the header or past the event; type outside 1..6; fewer
                                                    than 60 payload bytes; partitionId != partition_id; a DATA
                                                    message whose journal record is not a MESSAGE record */
#define BMQCRC_STORAGE_APPLY_DATA_RECORD 4       /* fewer than 8 bytes behind the journal record; DataHeader
                                                    headerWords or messageWords 0; header + options >= the record;
                                                    the record ends past the message; last byte not in 1..8 or
                                                    larger than what header and options leave */
#define BMQCRC_STORAGE_APPLY_TOO_MANY_MESSAGES 5 /* more than msg_cap messages; index: the lowest event whose
                                                    last message does not fit */
#define BMQCRC_STORAGE_APPLY_OUT_OF_SYNC 6       /* 4 x journalOffsetWords != journal_pos + 60 i; a lease id below
                                                    the predecessor's; the predecessor's lease id with another
                                                    sequence number than its + 1 (message 0's predecessor is the
                                                    write head; a higher lease id comes with any sequence
                                                    number); DATA: 8 x MessageOffsetDwords != data_file_pos + Q[i] */
#define BMQCRC_STORAGE_APPLY_DST_TOO_SMALL 7     /* 60 n_msgs > journal_dst_bytes or Q[n_msgs] > data_dst_bytes;
                                                    index: the lowest message ending past its destination, the
                                                    journal's before the DATA window's */
#define BMQCRC_STORAGE_APPLY_TOO_MANY_PIECES 8   /* beyond the copy kernel's 2^32-1 16-byte pieces per call */

typedef struct bmqcrc_storage_apply {
    uint32_t struct_size, reserved;       /* sizeof, 0 */
    const void* events;                   /* device, 4-byte aligned */
    uint64_t events_bytes;
    const uint64_t* event_offsets;        /* device, n_events + 1: event e is [event_offsets[e], event_offsets[e+1]);
                                             NULL = one event, the whole buffer (n_events must be 1) */
    uint64_t n_events;
    uint64_t msg_cap;                     /* capacity of the per-message arrays, < 2^32 */
    uint32_t partition_id;                /* <= 65535 */
    uint32_t lease_id;                    /* the write head; 0: none known yet */
    uint64_t seq;
    uint64_t journal_pos;                 /* byte of the journal file that journal_dst[0] stands for: multiple of 4, > 0 */
    uint64_t data_file_pos;               /* byte of the DATA file that data_dst[0] stands for: multiple of 8, > 0 */
    void* journal_dst;                    /* device, 4-byte aligned */
    uint64_t journal_dst_bytes;
    void* data_dst;                       /* device, 8-byte aligned */
    uint64_t data_dst_bytes;
    uint8_t* types;                       /* device, msg_cap, may be NULL: StorageMessageType */
    uint8_t* flags;                       /* device, msg_cap, may be NULL: StorageHeader flags (5 bits) */
    uint64_t* payload_offsets;            /* device, msg_cap, may be NULL: byte offset in `events` behind the journal record */
    uint32_t* payload_lengths;            /* device, msg_cap, may be NULL */
    uint64_t* record_offsets;             /* device, msg_cap + 1, may be NULL: Q, the total behind the last */
    uint32_t* lengths;                    /* device, msg_cap, may be NULL: application data bytes */
    uint32_t* expected;                   /* device, msg_cap, may be NULL: the stored CRCs, host order */
    uint32_t* out;                        /* device, msg_cap, may be NULL: the computed CRCs */
    uint64_t* event_first;                /* device, n_events + 1, may be NULL: first message of each event, n last */
} bmqcrc_storage_apply;

/* All fields zero before the first call on (device, stream); after a refused
 * call only n_events and the refused_* fields are set. */
typedef struct bmqcrc_storage_apply_result {
    uint64_t n_events, n_msgs, n_data;    /* n_data: DATA messages */
    uint64_t journal_bytes, data_bytes;   /* 60 n_msgs, Q[n_msgs] */
    uint64_t head_seq;                    /* the last message's sequence number and lease id: the new write head */
    uint32_t head_lease_id;               /* (the one given when there was no message) */
    uint32_t refused_kind;
    uint64_t n_bad, first_bad;            /* stored CRC != computed CRC; first_bad = n_msgs when none */
    uint64_t refused_event, refused_index, refused_offset;
} bmqcrc_storage_apply_result;

int bmqcrc_storage_event_apply(const bmqcrc_storage_apply* p, bmqcrc_storage_apply_result* result,
                               const bmqcrc_opts* opts);

/* ABI 2.15.  Result of the previous bmqcrc_storage_event_apply on (device,
 * stream); waits for it.  `result` may be NULL. */
int bmqcrc_last_storage_apply(int device, void* stream, bmqcrc_storage_apply_result* result);

/* ABI 2.16.  The primary's side of replication: journal records and the DATA
 * records they name, both in device memory, are packed ON THE DEVICE into the
 * STORAGE events the replicas receive -- FileStore::replicateRecord with
 * bmqp::StorageEventBuilder::packMessage for a batch of records in one
 * asynchronous call, byte for byte what the builder emits.  The application
 * data of every DATA message is moved by the fused copy of bmqcrc_crc32c_copy,
 * whose CRC32-C is compared with the one the MessageRecord stores ("verify on
 * send"), at the cost of the copy the primary has to make anyway.  No payload
 * byte and no descriptor crosses PCIe.
 *
 * Records.  Record i is journal[60 i .. 60 i + 60), i = 0 .. n_records - 1: the
 *   record run, not the journal file with its headers.  journal_pos is the byte
 *   of the journal file that record 0 stands for.  `data` is a window of the
 *   DATA file and data_file_pos the byte of that file that data[0] stands for,
 *   as in bmqcrc_message_records_unpack: a MESSAGE record's DATA record begins
 *   at byte o = 8 x MessageOffsetDwords (the BE u32 at byte 32) of the file,
 *   byte o - data_file_pos of the window.
 * One storage message per record, in record order.  Its StorageMessageType
 *   comes from the RecordType (the high 4 bits of byte 0):
 *     MESSAGE (1)     DATA (1), with its whole DATA record as payload:
 *                     DataHeader, option words, application data, 1..8 padding
 *                     bytes, R = 4 x DataHeader.messageWords bytes in all;
 *     CONFIRM (2)     CONFIRM (3);    DELETION (3)  DELETION (4);
 *     JOURNAL_OP (5)  JOURNAL_OP (5);
 *     QUEUE_OP (4)    by its QueueOpType, the BE u32 at byte 32: PURGE (1) or
 *                     DELETION (3) give QUEUE_OP (6); CREATION (2) or ADDITION
 *                     (4) give QLIST (2) CARRYING THE JOURNAL RECORD ONLY, which
 *                     is what FileStore::writeQueueCreationRecord hands
 *                     replicateRecord when the cluster is not QLIST aware.
 *   Not built: the QLIST file and a QLIST message's payload (the QLIST record)
 *   stay on the host, as in bmqcrc_storage_event_apply.  R = 0 for every record
 *   that is not a MESSAGE record.
 * Events.  Event e holds records [event_first[e], event_first[e + 1]);
 *   event_first has n_events + 1 entries, 0 first and n_records last, strictly
 *   increasing (no event is empty).  event_first == NULL means one event
 *   (n_events must be 1).  The caller cuts the events, as in
 *   bmqcrc_put_event_pack: a greedy fill to a size cap is a serial decision the
 *   broker makes by its own flush policy.
 * Layout.  With B[i] = 12 + 60 + R[i], P the 64-bit exclusive prefix of B and
 *   e(i) the event of message i: event e lies at dst + 8 e + P[event_first[e]],
 *   message i's StorageHeader at dst + 8 (e(i) + 1) + P[i], its journal record
 *   12 bytes behind that and its DATA record 72 bytes behind it.
 *   EventHeader (8 bytes): BE u32 length of the event (fragment bit 0); a byte
 *   (1 << 6) | event_type; a byte 2 (headerWords); two bytes 0.  event_type is
 *   STORAGE (8) or PARTITION_SYNC (10), 0 means STORAGE; PARTITION_SYNC is the
 *   same bytes under another type.
 *   StorageHeader (12 bytes): BE u32 (flags[i] & 31) << 27 | (18 + R[i] / 4); a
 *   byte (storage_protocol_version << 4) | 3; a byte StorageMessageType; BE u16
 *   partition_id; BE u32 JournalOffsetWords = (journal_pos + 60 i) / 4.
 *   flags == NULL means 0 for every record.  The reference sets bit 0
 *   (RECEIPT_REQUESTED) on DATA messages that want a receipt and 0 elsewhere;
 *   here the caller decides, for any type.
 *   The journal record and the DATA record's DataHeader, option words and
 *   padding bytes are copied as they are; the application data, which lies
 *   between header plus options and the padding, is moved by the fused copy.
 * Outputs, each may be NULL: event_offsets (n_events + 1 entries: the byte of
 *   dst where each event starts, the total behind the last), types[i] (the
 *   StorageMessageType chosen), out[i] (the computed CRC32-C of the application
 *   data, 0 for a record that is not a MESSAGE record).
 * Verify on send.  expected[i] is the MessageRecord's CRC, the BE u32 at byte 52.
 *   n_bad counts the MESSAGE records whose computed CRC differs, first_bad is the
 *   lowest (n_records when none).  A mismatch does not fail the call and the
 *   bytes go out as they are: whether to replicate them is the caller's decision.
 * All or nothing, decided on the device.  One violation anywhere refuses the
 *   call, and a refused call writes nothing to dst or to any output array.  The
 *   lowest kind wins and within it the lowest index (BMQCRC_STORAGE_PACK_* below;
 *   the index is a record, an event_first entry or an event, by kind).  The
 *   DATA-window checks are made in this order and no DATA byte is loaded before
 *   its range is shown to lie in the window.  EVENT_TOO_BIG, DST_TOO_SMALL and
 *   TOO_MANY_PIECES are evaluated only when no lower kind was raised.
 *   NOT checked: GUIDs, queue keys, the order of sequence numbers, queue
 *   liveness.  The primary wrote these records itself, and bmqcrc_journal_select
 *   holds those checks.  A synchronous call returns BMQCRC_EINVAL naming kind and
 *   index; after an asynchronous call bmqcrc_last_storage_pack reports them.
 * Caps.  max_event_bytes 0 means EventHeader::k_MAX_SIZE_SOFT (512 MiB), at most
 *   2^31 - 1; max_payload_bytes 0 means StorageHeader::k_MAX_PAYLOAD_SIZE_SOFT
 *   (65 MiB), at most 4 (2^27 - 1) - 12 so that MessageWords cannot overflow.
 * Options.  Device pointers only: BMQCRC_F_DEVICE_PTRS is required,
 *   BMQCRC_F_ASYNC allowed; any other flag, ndevices > 1, a wrong struct_size or
 *   a non-zero reserved field; journal, data or dst null; journal or dst not
 *   4-byte aligned, data not 8-byte aligned; journal_bytes != 60 n_records;
 *   event_first == NULL with n_events != 1; n_events outside [1, n_records] when
 *   n_records > 0; journal_pos 0 or no multiple of 4, or journal_pos + 60
 *   n_records above 4 (2^32 - 1); data_file_pos no multiple of 8; partition_id
 *   above 65535; event_type other than 0, 8 or 10; storage_protocol_version
 *   above 3; a cap above its limit; dst or an output array meeting an input
 *   (journal, data, flags, event_first), dst or another output array is
 *   BMQCRC_EINVAL, answered on the host before the device lookup.
 *   n_records == 0 launches nothing, writes nothing and reports zeros.
 * The copy runs over the n_records records (those that are not MESSAGE records
 *   are empty messages).  Nothing at or beyond dst_bytes, n_events + 1 entries
 *   of event_offsets or n_records entries of types and out is ever written.
 * *result (may be NULL) is written by a synchronous call only.
 * State.  As bmqcrc_storage_event_apply: takes the workspace mutex of (device,
 *   stream); restores the caller's current device; allocates its own workspace
 *   on first use and when n_records grows (41 bytes per record, none per event),
 *   which bmqcrc_reserve does not cover; is not meant to be captured into a
 *   hipGraph; is deterministic.  The copy's counters live in the call's own
 *   scratch: the shape prediction and the records of every other bmqcrc_last_*
 *   call are never touched. */
#define BMQCRC_STORAGE_PACK_OK 0
#define BMQCRC_STORAGE_PACK_RECORD_HEADER 1    /* BMQCRC_REC_UNPACK_RECORD_HEADER's conditions (type 0, lease id 0,
                                                  sequence number 0, a wrong magic); a type above 5; a QUEUE_OP
                                                  record whose QueueOpType is outside 1..4.  Index: the record */
#define BMQCRC_STORAGE_PACK_DATA_OFFSET 2      /* a MESSAGE record with o == 0, o < data_file_pos or
                                                  o - data_file_pos > data_bytes.  Index: the record */
#define BMQCRC_STORAGE_PACK_DATA_RECORD 3      /* a MESSAGE record with fewer than 8 bytes of window at its
                                                  offset; DataHeader headerWords or messageWords 0; header +
                                                  options >= the record; the record ends past the window; last
                                                  byte not in 1..8 or larger than what header and options leave.
                                                  Index: the record */
#define BMQCRC_STORAGE_PACK_EVENT_FIRST 4      /* event_first[0] != 0, event_first[e] >= event_first[e + 1] or
                                                  event_first[n_events] != n_records.  Index: the entry */
#define BMQCRC_STORAGE_PACK_PAYLOAD_TOO_BIG 5  /* 60 + R[i] > max_payload_bytes.  Index: the record */
#define BMQCRC_STORAGE_PACK_EVENT_TOO_BIG 6    /* an event longer than max_event_bytes.  Index: the event */
#define BMQCRC_STORAGE_PACK_DST_TOO_SMALL 7    /* index: the lowest event ending past dst_bytes */
#define BMQCRC_STORAGE_PACK_TOO_MANY_PIECES 8  /* beyond the copy kernel's 2^32-1 16-byte pieces per call: the sum
                                                  over the MESSAGE records with application data of
                                                  ((length + 15) >> 4) + 1.  Index 0 */

typedef struct bmqcrc_storage_pack {
    uint32_t struct_size, reserved;       /* sizeof, 0 */
    const void* journal;                  /* device, 4-byte aligned: n_records 60-byte records, the record run */
    uint64_t journal_bytes;               /* == 60 * n_records */
    uint64_t n_records;
    uint64_t journal_pos;                 /* byte of the journal file that record 0 stands for: multiple of 4, > 0 */
    const void* data;                     /* device, 8-byte aligned: the DATA-file window */
    uint64_t data_bytes;
    uint64_t data_file_pos;               /* byte of the DATA file that data[0] stands for: multiple of 8 */
    uint32_t partition_id;                /* <= 65535 */
    uint32_t event_type;                  /* 8 STORAGE, 10 PARTITION_SYNC, 0 = STORAGE */
    uint32_t storage_protocol_version;    /* <= 3 */
    uint32_t reserved2;                   /* 0 */
    const uint8_t* flags;                 /* device, n_records, may be NULL (all 0): StorageHeader flags, low 5 bits */
    const uint64_t* event_first;          /* device, n_events + 1; NULL = one event (n_events must be 1) */
    uint64_t n_events;
    uint64_t max_event_bytes;             /* 0 = 512 MiB; <= 2^31 - 1 */
    uint64_t max_payload_bytes;           /* 0 = 65 MiB; <= 4 (2^27 - 1) - 12 */
    void* dst;                            /* device, 4-byte aligned */
    uint64_t dst_bytes;
    uint64_t* event_offsets;              /* device, n_events + 1, may be NULL: the total behind the last */
    uint8_t* types;                       /* device, n_records, may be NULL: StorageMessageType */
    uint32_t* out;                        /* device, n_records, may be NULL: the computed CRCs */
} bmqcrc_storage_pack;

/* All fields zero before the first call on (device, stream); after a refused
 * call only n_events and the refused_* fields are set. */
typedef struct bmqcrc_storage_pack_result {
    uint64_t n_events, n_msgs, n_data;    /* n_msgs = n_records; n_data: DATA messages */
    uint64_t total_bytes;                 /* bytes of all events */
    uint64_t n_bad, first_bad;            /* stored CRC != computed CRC; first_bad = n_msgs when none */
    uint32_t refused_kind, reserved;
    uint64_t refused_index;               /* a record, an event_first entry or an event, by kind */
} bmqcrc_storage_pack_result;

int bmqcrc_storage_event_pack(const bmqcrc_storage_pack* p, bmqcrc_storage_pack_result* result,
                              const bmqcrc_opts* opts);

/* ABI 2.16.  Result of the previous bmqcrc_storage_event_pack on (device,
 * stream); waits for it.  `result` may be NULL. */
int bmqcrc_last_storage_pack(int device, void* stream, bmqcrc_storage_pack_result* result);

/* ABI 2.17.  Delivery to consumers: stored messages, journal and DATA records
 * both in device memory, are packed ON THE DEVICE into the PUSH events the
 * consumers receive -- mqba::ClientSession's delivery loop with
 * bmqp::PushEventBuilder::packMessage for a batch of messages in one
 * asynchronous call, byte for byte what the builder emits.  The application
 * data of every message is moved by the fused copy of bmqcrc_crc32c_copy, whose
 * CRC32-C is compared with the one the MessageRecord stores ("verify on
 * delivery", a check the reference never makes), at the cost of the copy the
 * broker has to make anyway.  No payload byte and no descriptor crosses PCIe.
 *
 * Records.  Record i is journal[60 i .. 60 i + 60), i = 0 .. n_records - 1, and
 *   `data` a window of the DATA file whose byte 0 stands for byte data_file_pos
 *   of that file, as in bmqcrc_storage_event_pack (alignment included).
 * Messages.  Message m, m = 0 .. n - 1, is journal record records[m], which must
 *   be a MESSAGE record.  The entries may come in any order and may repeat: a
 *   fan-out to several consumer handles is the same record under several queue
 *   ids.  records == NULL means message m is record m; n must then equal
 *   n_records (and every record be a MESSAGE record).  queue_ids[m] is the id
 *   the consumer opened the queue under.  flags[m] may carry
 *   PushHeaderFlags::e_OUT_OF_ORDER (4) and nothing else; flags == NULL means 0.
 *   e_MESSAGE_PROPERTIES (2) is taken from the DATA record; e_IMPLICIT_PAYLOAD
 *   is not supported.
 * Options.  One form per call (option_mode), so the option size O is uniform:
 *     0                 O = 0   none;
 *     1 PACKED_RDA      O = 4   one packed SUB_QUEUE_INFOS OptionHeader, BE u32
 *                               (3 << 26) | (1 << 25) | rda[m]: the default
 *                               sub-queue with its redelivery counter, what a
 *                               downstream broker gets in non-fan-out mode;
 *     2 SUB_QUEUE_ID    O = 8   SUB_QUEUE_IDS_OLD with one id, BE u32
 *                               (1 << 26) | 2, then BE u32 sub_ids[m]: what a
 *                               first-hop SDK client gets;
 *     3 SUB_QUEUE_INFO  O = 12  unpacked SUB_QUEUE_INFOS with one item, BE u32
 *                               (3 << 26) | (2 << 21) | 3, then BE u32
 *                               sub_ids[m], the byte rda[m], three bytes 0.
 *   These are the forms of PushEventBuilder::addSubQueueInfosOption for one
 *   sub-queue.  rda (u8 per message) is required in modes 1 and 3, sub_ids (u32
 *   per message) in modes 2 and 3; an array the mode does not use must be NULL.
 * Events.  Event e holds messages [event_first[e], event_first[e + 1]), as in
 *   bmqcrc_storage_event_pack: n_events + 1 entries, 0 first and n last,
 *   strictly increasing; NULL means one event (n_events must be 1).  The caller
 *   cuts the events.
 * Layout.  With L[m] the application data's length, pad(L) = 4 - L % 4 (1..4
 *   bytes, each equal to the count; L = 0 gives four bytes of 4), B[m] = 32 + O +
 *   L[m] + pad(L[m]), P the 64-bit exclusive prefix of B and e(m) the event of
 *   message m: event e lies at dst + 8 e + P[event_first[e]], message m's
 *   PushHeader at dst + 8 (e(m) + 1) + P[m], its option 32 bytes behind that and
 *   its application data 32 + O bytes behind it.
 *   EventHeader (8 bytes): BE u32 length of the event (fragment bit 0); a byte
 *   (1 << 6) | 4 (PUSH); a byte 2 (headerWords); two bytes 0.
 *   PushHeader (32 bytes): BE u32 F << 28 | (8 + O / 4 + (L + pad) / 4); BE u32
 *   (O / 4) << 8 | CAT << 5 | 8; BE i32 queue_ids[m]; the 16 GUID bytes of the
 *   MessageRecord (bytes 36..51); two SchemaId bytes; two bytes 0.  CAT is the
 *   low 3 bits of MessageRecord byte 21; F is (flags[m] & 4) |
 *   (DataHeader.flags & 1 ? 2 : 0); SchemaId is DataHeader bytes 8..9 when its
 *   headerWords >= 3, else 0: MessagePropertiesInfo(dataHeader).applyTo(
 *   pushHeader) and the attributes FileStore::get returns.
 *   The application data is the DATA record minus DataHeader, option words and
 *   padding, moved as stored: compressed bytes stay compressed and the CRC is
 *   over them, as the PUT header's was.  A DATA record's own option words are
 *   skipped, not forwarded.
 * Outputs, each may be NULL: event_offsets (n_events + 1 entries: the byte of
 *   dst where each event starts, the total behind the last), out[m] (the
 *   computed CRC32-C of the application data), lengths[m] (L[m]).
 * Verify on delivery.  The stored CRC is the MessageRecord's BE u32 at byte 52.
 *   n_bad counts the messages whose computed CRC differs, first_bad is the
 *   lowest (n when none).  A mismatch does not fail the call and the bytes go
 *   out as they are: whether to deliver them is the caller's decision.
 * Size only.  dst == NULL with dst_bytes == 0 runs the layout and every check
 *   except DST_TOO_SMALL, writes event_offsets and the result (total_bytes) and
 *   nothing else (n_bad is 0, first_bad n), and launches neither the copy nor
 *   the frame.  With repeats allowed the size of `data` gives no bound on dst:
 *   this is how a caller sizes it exactly.
 * All or nothing, decided on the device.  One violation anywhere refuses the
 *   call, and a refused call writes nothing to dst or to any output array.  The
 *   lowest kind wins and within it the lowest index (BMQCRC_PUSH_PACK_* below;
 *   the index is a message, an event_first entry or an event, by kind).  No
 *   journal byte outside the run is loaded and no DATA byte before its range is
 *   shown to lie in the window.  EVENT_TOO_BIG, DST_TOO_SMALL and
 *   TOO_MANY_PIECES are evaluated only when no lower kind was raised.  A
 *   synchronous call returns BMQCRC_EINVAL naming kind and index; after an
 *   asynchronous call bmqcrc_last_push_pack reports them.
 * Caps.  max_event_bytes 0 means EventHeader::k_MAX_SIZE_SOFT (512 MiB), at most
 *   2^31 - 1; max_payload_bytes 0 means PushHeader::k_MAX_PAYLOAD_SIZE_SOFT
 *   (64 MiB), at most 4 (2^28 - 1) - 32 - 12 - 4 so that MessageWords (28 bits)
 *   cannot overflow.
 * Options of the call.  Device pointers only: BMQCRC_F_DEVICE_PTRS is required,
 *   BMQCRC_F_ASYNC allowed; any other flag, ndevices > 1, a wrong struct_size or
 *   a non-zero reserved field; journal, data or queue_ids null; dst null with
 *   dst_bytes != 0; journal or dst not 4-byte aligned, data not 8-byte aligned;
 *   journal_bytes != 60 n_records; n >= 2^32; records == NULL with n !=
 *   n_records; event_first == NULL with n_events != 1; n_events outside [1, n]
 *   when n > 0; data_file_pos no multiple of 8; option_mode above 3; an rda or
 *   sub_ids pointer that does not fit the mode; a cap above its limit; dst or an
 *   output array meeting an input (journal, data, records, queue_ids, flags,
 *   rda, sub_ids, event_first), dst or another output array is BMQCRC_EINVAL,
 *   answered on the host before the device lookup.
 *   n == 0 launches nothing, writes nothing and reports zeros.
 * The copy runs over the n messages.  Nothing at or beyond dst_bytes, n_events +
 *   1 entries of event_offsets or n entries of out and lengths is ever written.
 * *result (may be NULL) is written by a synchronous call only.
 * State.  As bmqcrc_storage_event_pack: takes the workspace mutex of (device,
 *   stream); restores the caller's current device; allocates its own workspace
 *   on first use and when n grows (36 bytes per message, none per event), which
 *   bmqcrc_reserve does not cover; is not meant to be captured into a hipGraph;
 *   is deterministic.  The copy's counters live in the call's own scratch: the
 *   shape prediction and the records of every other bmqcrc_last_* call are never
 *   touched. */
#define BMQCRC_PUSH_PACK_OK 0
#define BMQCRC_PUSH_PACK_RECORD_INDEX 1     /* records[m] >= n_records.  Index: the message */
#define BMQCRC_PUSH_PACK_RECORD 2           /* BMQCRC_REC_UNPACK_RECORD_HEADER's conditions (type 0, lease id 0,
                                               sequence number 0, a wrong magic), or the record's type is not
                                               MESSAGE.  Index: the message */
#define BMQCRC_PUSH_PACK_DATA_OFFSET 3      /* BMQCRC_STORAGE_PACK_DATA_OFFSET's conditions.  Index: the message */
#define BMQCRC_PUSH_PACK_DATA_RECORD 4      /* BMQCRC_STORAGE_PACK_DATA_RECORD's conditions.  Index: the message */
#define BMQCRC_PUSH_PACK_FLAGS 5            /* flags[m] has a bit other than 4.  Index: the message */
#define BMQCRC_PUSH_PACK_EVENT_FIRST 6      /* event_first[0] != 0, event_first[e] >= event_first[e + 1] or
                                               event_first[n_events] != n.  Index: the entry */
#define BMQCRC_PUSH_PACK_PAYLOAD_TOO_BIG 7  /* L[m] > max_payload_bytes.  Index: the message */
#define BMQCRC_PUSH_PACK_EVENT_TOO_BIG 8    /* an event longer than max_event_bytes.  Index: the event */
#define BMQCRC_PUSH_PACK_DST_TOO_SMALL 9    /* index: the lowest event ending past dst_bytes */
#define BMQCRC_PUSH_PACK_TOO_MANY_PIECES 10 /* beyond the copy kernel's 2^32-1 16-byte pieces per call: the sum
                                               over the messages with application data of
                                               ((length + 15) >> 4) + 1.  Index 0 */

#define BMQCRC_PUSH_OPTION_NONE 0
#define BMQCRC_PUSH_OPTION_PACKED_RDA 1
#define BMQCRC_PUSH_OPTION_SUB_QUEUE_ID 2
#define BMQCRC_PUSH_OPTION_SUB_QUEUE_INFO 3

typedef struct bmqcrc_push_pack {
    uint32_t struct_size, reserved;       /* sizeof, 0 */
    const void* journal;                  /* device, 4-byte aligned: n_records 60-byte records, the record run */
    uint64_t journal_bytes;               /* == 60 * n_records */
    uint64_t n_records;
    const void* data;                     /* device, 8-byte aligned: the DATA-file window */
    uint64_t data_bytes;
    uint64_t data_file_pos;               /* byte of the DATA file that data[0] stands for: multiple of 8 */
    const uint32_t* records;              /* device, n; NULL = message m is record m (n must be n_records) */
    uint64_t n;                           /* messages, < 2^32 */
    const int32_t* queue_ids;             /* device, n */
    const uint8_t* flags;                 /* device, n, may be NULL (all 0): only e_OUT_OF_ORDER (4) */
    uint32_t option_mode;                 /* BMQCRC_PUSH_OPTION_* */
    uint32_t reserved2;                   /* 0 */
    const uint8_t* rda;                   /* device, n: modes 1 and 3, NULL otherwise */
    const uint32_t* sub_ids;              /* device, n: modes 2 and 3, NULL otherwise */
    const uint64_t* event_first;          /* device, n_events + 1; NULL = one event (n_events must be 1) */
    uint64_t n_events;
    uint64_t max_event_bytes;             /* 0 = 512 MiB; <= 2^31 - 1 */
    uint64_t max_payload_bytes;           /* 0 = 64 MiB; <= 4 (2^28 - 1) - 48 */
    void* dst;                            /* device, 4-byte aligned; NULL with dst_bytes 0: size only */
    uint64_t dst_bytes;
    uint64_t* event_offsets;              /* device, n_events + 1, may be NULL: the total behind the last */
    uint32_t* out;                        /* device, n, may be NULL: the computed CRCs */
    uint32_t* lengths;                    /* device, n, may be NULL: the application data's lengths */
} bmqcrc_push_pack;

/* All fields zero before the first call on (device, stream); after a refused
 * call only n_events and the refused_* fields are set. */
typedef struct bmqcrc_push_pack_result {
    uint64_t n_events, n_msgs;            /* n_msgs = n */
    uint64_t total_bytes;                 /* bytes of all events */
    uint64_t n_bad, first_bad;            /* stored CRC != computed CRC; first_bad = n_msgs when none */
    uint32_t refused_kind, reserved;
    uint64_t refused_index;               /* a message, an event_first entry or an event, by kind */
} bmqcrc_push_pack_result;

int bmqcrc_push_event_pack(const bmqcrc_push_pack* p, bmqcrc_push_pack_result* result,
                           const bmqcrc_opts* opts);

/* ABI 2.17.  Result of the previous bmqcrc_push_event_pack on (device, stream);
 * waits for it.  `result` may be NULL. */
int bmqcrc_last_push_pack(int device, void* stream, bmqcrc_push_pack_result* result);

/* ABI 2.18.  Compaction: the outstanding records of a device-resident
 * partition, journal run and DATA window both in device memory, are rolled over
 * ON THE DEVICE into a new journal run and a new DATA window -- the loop of
 * FileStore::rolloverImpl over FileStore::writeRolledOverRecord and the sync
 * point it writes behind it, in one asynchronous call, byte for byte what the
 * reference's loop writes when its d_records holds exactly the kept records in
 * run order, in a cluster that is not QLIST aware.  The application data of
 * every kept message is moved by the fused copy of bmqcrc_crc32c_copy, whose
 * CRC32-C is compared with the one the MessageRecord stores ("verify on
 * rollover", a check the reference never makes: a byte that rots in the old
 * DATA file is carried into the new one), at the cost of the copy the rollover
 * has to make anyway.  No payload byte and no descriptor crosses PCIe.
 *
 * Records.  Record i is journal[60 i .. 60 i + 60), i = 0 .. n_records - 1, and
 *   `data` a window of the DATA file whose byte 0 stands for byte data_file_pos
 *   of that file, as in bmqcrc_storage_event_pack (alignment included).
 * Which records are kept.  keep[i] != 0 keeps record i; keep == NULL keeps
 *   every record that may be kept.  For MESSAGE records keep is exactly the
 *   select array of bmqcrc_journal_select.  A JOURNAL_OP record is never rolled:
 *   keep[i] != 0 on one refuses the call (keep == NULL: it is not kept).  What
 *   is outstanding is the caller's decision, with one exception:
 *   confirm_mode BMQCRC_ROLLOVER_CONFIRMS_AS_KEPT (0): keep decides CONFIRM
 *     records like the others;
 *   confirm_mode BMQCRC_ROLLOVER_CONFIRMS_FOLLOW_MESSAGES (1): a CONFIRM record
 *     is kept if and only if some kept MESSAGE record of the run has the same
 *     GUID (bytes 36..51 of the MESSAGE record, 32..47 of the CONFIRM record)
 *     and the same queue key (bytes 22..26 of both), wherever in the run it
 *     lies; keep[] is ignored for CONFIRM records.  The live broker's rule
 *     (FileBackedStorage keeps a message's CONFIRM handles with its MESSAGE
 *     handle and removes them together): with it bmqcrc_journal_select ->
 *     bmqcrc_partition_rollover needs no per-record work on the host for the
 *     two record types that exist per message.  QUEUE_OP and DELETION records
 *     stay with the caller.
 * What is written.  With R[i] = 4 DataHeader.messageWords of a kept MESSAGE
 *   record (0 for every other record), Q the 64-bit exclusive prefix of R and J
 *   the exclusive prefix of "kept": record i goes to journal_dst + 60 J[i].
 *   A kept MESSAGE record's whole DATA record (DataHeader, option words,
 *   application data, padding) is copied to dst + Q[i] -- the DataHeader, option
 *   words and padding bytes as they are, the application data by the fused copy
 *   -- and its journal record with the BE u32 at byte 32 (MessageOffsetDwords)
 *   set to (new_data_file_pos + Q[i]) / 8.  Two kept MESSAGE records that name
 *   one DATA record each get a copy of their own.  A kept QUEUE_OP CREATION (2)
 *   or ADDITION (4) record is copied with the BE u32 at byte 36
 *   (queueUriRecordOffsetWords) set to 0; PURGE / DELETION QUEUE_OP records,
 *   CONFIRM and DELETION records are copied as they are.
 * Sync point.  With sync_point != BMQCRC_ROLLOVER_NO_SYNC_POINT one more record
 *   follows the last kept one, built from record s = sync_point, which must be
 *   a JOURNAL_OP record of JournalOpType SYNCPOINT: BE u16 0x5000; bytes 2..11
 *   of s (sequence number, lease id); BE u64 timestamp at 12; bytes 20..22 zero;
 *   byte 23 = 1 (REGULAR); BE u32 2 (SYNCPOINT) at 24; bytes 28..43 of s
 *   (sequence number, primary node id, primary lease id); BE u32
 *   (new_data_file_pos + Q[n_records]) / 8 at 44; bytes 48..55 zero; the magic
 *   0x2A724563 at 56.  Setting JournalFileHeader.
 *   firstSyncPointAfterRolloverOffsetWords stays with the caller, who owns the
 *   file headers.  Every other sync point is dropped, as the reference drops it.
 * Not built: the QLIST file; the file headers of the new files.
 * Outputs, each may be NULL: new_index[i] (J[i], 0xFFFFFFFF for a record not
 *   kept), out[i] (the computed CRC32-C of a kept MESSAGE record's application
 *   data, 0 elsewhere).
 * Verify on rollover.  The stored CRC is the MessageRecord's BE u32 at byte 52.
 *   n_bad counts the kept MESSAGE records whose computed CRC differs, first_bad
 *   is the lowest (n_records when none).  A mismatch does not fail the call and
 *   the bytes are rolled as they are: what to do about it is the caller's
 *   decision.
 * All or nothing, decided on the device.  One violation anywhere refuses the
 *   call, and a refused call writes nothing to dst, journal_dst or any output
 *   array.  The lowest kind wins and within it the lowest index
 *   (BMQCRC_ROLLOVER_* below).  No DATA byte of a record that is not kept is
 *   ever loaded, and no DATA byte before its range is shown to lie in the
 *   window.  DST_TOO_SMALL, DATA_FILE_FULL and TOO_MANY_PIECES are evaluated
 *   only when no lower kind was raised.  NOT checked: GUIDs, queue keys, the
 *   order of sequence numbers, queue liveness: bmqcrc_journal_select holds
 *   those checks.  A synchronous call returns BMQCRC_EINVAL naming kind and
 *   index; after an asynchronous call bmqcrc_last_rollover reports them.
 * Options.  Device pointers only: BMQCRC_F_DEVICE_PTRS is required,
 *   BMQCRC_F_ASYNC allowed; any other flag, ndevices > 1, a wrong struct_size or
 *   a non-zero reserved field; journal, data, dst or journal_dst null; journal,
 *   journal_dst, new_index or out not 4-byte aligned, data or dst not 8-byte
 *   aligned; journal_bytes != 60 n_records; n_records >= 2^32; data_file_pos no
 *   multiple of 8; new_data_file_pos 0 or no multiple of 8; confirm_mode above
 *   1; sync_point neither below n_records nor BMQCRC_ROLLOVER_NO_SYNC_POINT;
 *   dst, journal_dst or an output array meeting an input (journal, data, keep)
 *   or one another is BMQCRC_EINVAL, answered on the host before the device
 *   lookup.  n_records == 0 (which admits no sync point) launches nothing,
 *   writes nothing and reports zeros.
 * The copy runs over the n_records records (those that are not kept MESSAGE
 *   records are empty messages).  Nothing at or beyond dst_bytes,
 *   journal_dst_bytes or n_records entries of new_index and out is ever written.
 * *result (may be NULL) is written by a synchronous call only.
 * State.  As bmqcrc_storage_event_pack: takes the workspace mutex of (device,
 *   stream); restores the caller's current device; allocates its own workspace
 *   on first use and when n_records grows (49 bytes per record, and in
 *   FOLLOW mode 8 to 16 more for the hash), which bmqcrc_reserve does not
 *   cover; is not meant to be captured into a hipGraph; is deterministic.  The
 *   copy's counters live in the call's own scratch: the shape prediction and
 *   the records of every other bmqcrc_last_* call are never touched. */
#define BMQCRC_ROLLOVER_OK 0
#define BMQCRC_ROLLOVER_RECORD_HEADER 1    /* BMQCRC_REC_UNPACK_RECORD_HEADER's conditions (type 0, lease id 0,
                                              sequence number 0, a wrong magic); a type above 5; a QUEUE_OP
                                              record whose QueueOpType is outside 1..4 -- on every record
                                              of the run, kept or not.  Index: the record */
#define BMQCRC_ROLLOVER_KEEP_JOURNAL_OP 2  /* keep[i] != 0 on a JOURNAL_OP record.  Index: the record */
#define BMQCRC_ROLLOVER_SYNC_POINT 3       /* record sync_point is not a JOURNAL_OP record of JournalOpType
                                              SYNCPOINT.  Index: sync_point */
#define BMQCRC_ROLLOVER_DATA_OFFSET 4      /* BMQCRC_STORAGE_PACK_DATA_OFFSET's conditions, on kept MESSAGE
                                              records only.  Index: the record */
#define BMQCRC_ROLLOVER_DATA_RECORD 5      /* BMQCRC_STORAGE_PACK_DATA_RECORD's conditions, on kept MESSAGE
                                              records only.  Index: the record */
#define BMQCRC_ROLLOVER_DST_TOO_SMALL 6    /* index: the lowest kept record whose DATA record ends past
                                              dst_bytes or whose journal record ends past
                                              journal_dst_bytes; n_records: the sync point does */
#define BMQCRC_ROLLOVER_DATA_FILE_FULL 7   /* index: the lowest kept MESSAGE record whose DATA record ends
                                              past byte 8 (2^32 - 1) of the new DATA file; n_records:
                                              new_data_file_pos itself lies past it */
#define BMQCRC_ROLLOVER_TOO_MANY_PIECES 8  /* beyond the copy kernel's 2^32-1 16-byte pieces per call: the sum
                                              over the kept MESSAGE records with application data of
                                              ((length + 15) >> 4) + 1.  Index 0 */

#define BMQCRC_ROLLOVER_CONFIRMS_AS_KEPT 0
#define BMQCRC_ROLLOVER_CONFIRMS_FOLLOW_MESSAGES 1
#define BMQCRC_ROLLOVER_NO_SYNC_POINT 0xFFFFFFFFFFFFFFFFull

typedef struct bmqcrc_rollover {
    uint32_t struct_size, reserved;       /* sizeof, 0 */
    const void* journal;                  /* device, 4-byte aligned: n_records 60-byte records, the record run */
    uint64_t journal_bytes;               /* == 60 * n_records */
    uint64_t n_records;                   /* < 2^32 */
    const void* data;                     /* device, 8-byte aligned: the DATA-file window */
    uint64_t data_bytes;
    uint64_t data_file_pos;               /* byte of the DATA file that data[0] stands for: multiple of 8 */
    const uint8_t* keep;                  /* device, n_records, may be NULL (every record that may be kept) */
    uint32_t confirm_mode;                /* BMQCRC_ROLLOVER_CONFIRMS_* */
    uint32_t reserved2;                   /* 0 */
    uint64_t sync_point;                  /* the record restated behind the kept ones, or ..._NO_SYNC_POINT */
    uint64_t timestamp;                   /* the restated sync point's */
    uint64_t new_data_file_pos;           /* byte of the NEW DATA file that dst[0] stands for: multiple of 8, > 0 */
    void* dst;                            /* device, 8-byte aligned: the DATA records back to back */
    uint64_t dst_bytes;
    void* journal_dst;                    /* device, 4-byte aligned: the 60-byte records back to back */
    uint64_t journal_dst_bytes;
    uint32_t* new_index;                  /* device, n_records, may be NULL: position in the new run */
    uint32_t* out;                        /* device, n_records, may be NULL: the computed CRCs */
} bmqcrc_rollover;

/* All fields zero before the first call on (device, stream); after a refused
 * call only n_records and the refused_* fields are set. */
typedef struct bmqcrc_rollover_result {
    uint64_t n_records, n_kept, n_messages; /* n_kept: records rolled, the sync point not counted;
                                               n_messages: MESSAGE records among them */
    uint64_t journal_bytes, data_bytes;   /* bytes written to journal_dst (the sync point included) and dst */
    uint64_t n_bad, first_bad;            /* stored CRC != computed CRC; first_bad = n_records when none */
    uint32_t refused_kind, reserved;
    uint64_t refused_index;               /* a record, or n_records, by kind */
} bmqcrc_rollover_result;

int bmqcrc_partition_rollover(const bmqcrc_rollover* p, bmqcrc_rollover_result* result,
                              const bmqcrc_opts* opts);

/* ABI 2.18.  Result of the previous bmqcrc_partition_rollover on (device,
 * stream); waits for it.  `result` may be NULL. */
int bmqcrc_last_rollover(int device, void* stream, bmqcrc_rollover_result* result);

/* ABI 2.19.  The consumer's confirm: a batch of confirms, in device memory,
 * against the journal run of a device-resident partition becomes ON THE DEVICE
 * the CONFIRM and DELETION records the reference would append -- the path
 * QueueHandle::confirmMessage -> FileBackedStorage::confirm ->
 * FileStore::writeConfirmRecord and, when a message's count reaches zero,
 * FileBackedStorage::remove -> FileStore::writeDeletionRecord -- byte for byte,
 * in one asynchronous call.  THIS CALL HAS NO CRC IN IT: a confirm carries no
 * payload.  It is here because a device-resident partition that cannot record
 * a confirm cannot free anything.
 *
 * The journal is the state.  Nothing persists between calls: the outstanding
 *   count of every message is derived from the run, as recovery derives it
 *   (processMessageRecord / processConfirmRecord).  Record r is
 *   journal[60 r .. 60 r + 60), r = 0 .. n_records - 1.  select[r] != 0 selects
 *   MESSAGE record r (the output of bmqcrc_journal_select; on other records it
 *   is ignored); select == NULL selects every MESSAGE record.  With key = (GUID,
 *   queue key) -- bytes 36..51 and 22..26 of a MESSAGE record, 32..47 and 22..26
 *   of a CONFIRM record, 28..43 and 23..27 of a DELETION record:
 *   - a MESSAGE record m is LIVE if it is selected and no DELETION record
 *     anywhere in the run has its key;
 *   - had(m) is the number of CONFIRM records in the run with m's key whose
 *     ConfirmReason (the low 12 bits of the RecordHeader's flags) is not
 *     AUTO_CONFIRMED (2);
 *   - left(m) = max(refCount(m) - had(m), 0), refCount the 20-bit field
 *     (byte 20 above the RecordHeader's 12 flag bits); 0 when m is not live;
 *   - CONFIRM and DELETION records that name no selected MESSAGE record are
 *     ignored, as the reference logs and ignores them.
 *   Appending the call's output to the run and calling again needs no other
 *   bookkeeping: journal_dst may be journal + 60 n_records of one allocation.
 * The batch.  Confirm i = 0 .. n - 1 is guids[16 i .. +16), queue_keys[5 i ..
 *   +5), app_keys[5 i .. +5) (NULL: the null key), reasons[i] (0 CONFIRMED or 1
 *   REJECTED; NULL: 0) and timestamps[i] (NULL: `timestamp` for all).
 * What is written.  target(i) is the live MESSAGE record with confirm i's key,
 *   or none; c(m) the confirms of this call whose target is m; last(m) the
 *   highest of them.
 *   - No target: nothing is written, status[i] = 2 (the reference's
 *     e_GUID_NOT_FOUND, normal traffic after a consumer reconnects).
 *   - Otherwise confirm i writes one record at journal_dst + 60 j, j the number
 *     of confirms below i that have a target, with sequence number first_seq +
 *     j, lease_id and confirm i's timestamp:
 *     a DELETION record when i == last(m) and c(m) == left(m) (status[i] = 1):
 *       flags 0, the queue key at byte 23, the GUID at byte 28 -- the reference
 *       does not record the confirm that brings the count to zero and writes
 *       the DELETION in its place;
 *     a CONFIRM record otherwise (status[i] = 0): the reason in the flags, the
 *       queue key at byte 22, the app key at 27, the GUID at 32.
 *     Every other byte behind the RecordHeader is zero, the magic 0x2A724563 at 56.
 * Outputs, each may be NULL: status[n]; target[n] (the record index,
 *   0xFFFFFFFF for none); new_index[n] (j, or 0xFFFFFFFF); left_out[n_records]
 *   (left(m) - c(m) for MESSAGE records, 0 elsewhere: left_out > 0 is the next
 *   select).
 * Size only.  journal_dst == NULL with journal_dst_bytes == 0: everything is
 *   decided, nothing is stored (no output array either) and the result says
 *   what a real call would write.
 * All or nothing, decided on the device.  One violation anywhere refuses the
 *   call, and a refused call writes nothing.  The lowest kind wins and within
 *   it the lowest index (BMQCRC_CONFIRM_PACK_* below), whatever the order the
 *   device works in.  A synchronous call returns BMQCRC_EINVAL naming kind and
 *   index; after an asynchronous call bmqcrc_last_confirm_records reports them.
 * What differs from the reference.
 *   - Over-confirming within one call (c(m) > left(m)) is a refusal.  The
 *     reference would apply the first left(m) confirms and answer
 *     e_GUID_NOT_FOUND to the rest; deciding "first" needs each confirm's rank
 *     among the confirms of its message, which is not built.  Across calls the
 *     behaviour is the reference's: the later confirm finds no live message.
 *   - A mismatched app key is not detected: the per-app virtual storage stays
 *     with the caller, app_keys are copied into the records and nothing more.
 *   - The DELETION record takes the zeroing confirm's timestamp, where the
 *     reference reads the clock again.
 *   - There is no auto-confirm and no rollover-if-needed.
 *   - Nothing is replicated: the output goes to bmqcrc_storage_event_pack.
 * Options.  Device pointers only: BMQCRC_F_DEVICE_PTRS is required,
 *   BMQCRC_F_ASYNC allowed; any other flag, ndevices > 1, a wrong struct_size or
 *   a non-zero reserved field; journal, guids or queue_keys null; journal_dst
 *   null with journal_dst_bytes != 0; journal, journal_dst, target, new_index or
 *   left_out not 4-byte aligned, timestamps not 8-byte aligned; journal_bytes !=
 *   60 n_records; n or n_records >= 2^32; lease_id 0; first_seq 0 or first_seq
 *   + n above 2^48 - 1; journal_dst or an output array meeting an input or one
 *   another is BMQCRC_EINVAL, answered on the host before the device lookup.
 *   n == 0 launches nothing, writes nothing and reports zeros.
 * *result (may be NULL) is written by a synchronous call only.
 * State.  As bmqcrc_partition_rollover: takes the workspace mutex of (device,
 *   stream); restores the caller's current device; allocates its own workspace
 *   on first use and when the call grows (18 bytes per record and 8 to 16 more
 *   for the hash, 12 per confirm), which bmqcrc_reserve does not cover; is not
 *   meant to be captured into a hipGraph; is deterministic.  The shape
 *   prediction and the records of every other bmqcrc_last_* call are never
 *   touched. */
#define BMQCRC_CONFIRM_PACK_OK 0
#define BMQCRC_CONFIRM_PACK_RECORD_HEADER 1      /* BMQCRC_ROLLOVER_RECORD_HEADER's conditions, on every
                                                    record of the run.  Index: the record */
#define BMQCRC_CONFIRM_PACK_DUPLICATE_MESSAGE 2  /* two selected MESSAGE records share a key.  Index: the
                                                    lowest record among all that share theirs */
#define BMQCRC_CONFIRM_PACK_NULL_KEY 3           /* a confirm whose GUID or queue key is all zero.  Index:
                                                    the confirm */
#define BMQCRC_CONFIRM_PACK_REASON 4             /* reasons[i] above 1.  Index: the confirm */
#define BMQCRC_CONFIRM_PACK_OVER_CONFIRMED 5     /* c(m) > left(m).  Index: the lowest confirm whose
                                                    target is such a message */
#define BMQCRC_CONFIRM_PACK_DST_TOO_SMALL 6      /* index: the lowest confirm whose record ends past
                                                    journal_dst_bytes */

typedef struct bmqcrc_confirm_pack {
    uint32_t struct_size, reserved;       /* sizeof, 0 */
    const void* journal;                  /* device, 4-byte aligned: n_records 60-byte records, the record run */
    uint64_t journal_bytes;               /* == 60 * n_records */
    uint64_t n_records;                   /* < 2^32 */
    const uint8_t* select;                /* device, n_records, may be NULL (every MESSAGE record) */
    const uint8_t* guids;                 /* device, 16 n */
    const uint8_t* queue_keys;            /* device, 5 n */
    const uint8_t* app_keys;              /* device, 5 n, may be NULL (the null key) */
    const uint8_t* reasons;               /* device, n, may be NULL (all CONFIRMED) */
    const uint64_t* timestamps;           /* device, n, may be NULL (`timestamp` for all) */
    uint64_t n;                           /* confirms, < 2^32 */
    uint64_t timestamp;
    uint64_t first_seq;                   /* sequence number of the first record written, not 0 */
    uint32_t lease_id;                    /* primary lease id, not 0 */
    uint32_t reserved2;                   /* 0 */
    void* journal_dst;                    /* device, 4-byte aligned: the 60-byte records back to back;
                                             NULL (journal_dst_bytes 0): size only */
    uint64_t journal_dst_bytes;
    uint8_t* status;                      /* device, n, may be NULL: 0 CONFIRM, 1 DELETION, 2 not found */
    uint32_t* target;                     /* device, n, may be NULL */
    uint32_t* new_index;                  /* device, n, may be NULL */
    uint32_t* left_out;                   /* device, n_records, may be NULL */
} bmqcrc_confirm_pack;

/* All fields zero before the first call on (device, stream); after a refused
 * call only n_confirms and the refused_* fields are set. */
typedef struct bmqcrc_confirm_pack_result {
    uint64_t n_confirms;                  /* n */
    uint64_t n_written;                   /* records: n_confirm_records + n_deletions */
    uint64_t n_confirm_records, n_deletions, n_not_found;
    uint64_t journal_bytes;               /* 60 n_written */
    uint64_t next_seq;                    /* first_seq + n_written */
    uint32_t refused_kind, reserved;
    uint64_t refused_index;               /* a record or a confirm, by kind */
} bmqcrc_confirm_pack_result;

int bmqcrc_confirm_records_pack(const bmqcrc_confirm_pack* p, bmqcrc_confirm_pack_result* result,
                                const bmqcrc_opts* opts);

/* ABI 2.19.  Result of the previous bmqcrc_confirm_records_pack on (device,
 * stream); waits for it.  `result` may be NULL. */
int bmqcrc_last_confirm_records(int device, void* stream, bmqcrc_confirm_pack_result* result);

/* ABI 2.20.  The TTL: the messages of a device-resident partition whose
 * time-to-live has run out become ON THE DEVICE the DELETION records the
 * primary's garbage collection would append -- FileStore::gcExpiredMessages ->
 * FileBackedStorage::gcExpiredMessages -> FileStore::writeDeletionRecord with
 * DeletionRecordFlag::e_TTL_EXPIRATION -- byte for byte, in one asynchronous
 * call.  THIS CALL HAS NO CRC IN IT: no payload byte is read.  It is here
 * because a queue whose consumers are slow or gone would otherwise fill a
 * device-resident partition for ever.
 *
 * The journal is the state, as in bmqcrc_confirm_records_pack: the run, select
 *   and key = (GUID, queue key) mean what they mean there.
 *   - live(m): MESSAGE record m is selected and no DELETION record anywhere in
 *     the run has its key.  Reference counts play no part: the reference's loop
 *     walks every message it still holds.
 * The queue table is the domain configuration the reference holds per storage
 *   as d_ttlSeconds: entry q = 0 .. n_queues - 1 is queue_keys[5 q .. +5) and
 *   ttl_seconds[q].  n_queues == 0 is legal: nothing can expire.
 *   - queue(m): the entry whose 5 bytes equal bytes 22..26 of m, or none.  A
 *     live message without an entry is never expired and is counted in
 *     n_no_queue: the reference would have no storage to walk for it.
 *   - ts(m): bytes 12..19 of the record, big-endian: the RecordHeader's
 *     timestamp.
 *   - young(m): live(m), queue(m) = q exists and (now - ts(m)) mod 2^64 <=
 *     ttl_seconds[q].  The subtraction is unsigned and wraps, exactly as the
 *     reference's: a timestamp in the future reads as expired, unless an older
 *     young message stands before it.
 *   - front(q): the lowest record index of a young message of q, or n_records
 *     when there is none.
 *   - expired(m): live(m), queue(m) = q and m < front(q).
 *   This is the reference's loop restated without order: it deletes from the
 *   head of a queue's messages in arrival order and breaks at the first one
 *   that has not expired, so younger-looking stragglers behind it survive.
 *   After recovery, arrival order is journal order.
 * What is written.  The j-th expired MESSAGE record in journal order writes a
 *   DELETION record at journal_dst + 60 j: type 3, flags 2 (e_TTL_EXPIRATION),
 *   sequence number first_seq + j, lease_id, timestamp `now`, the queue key at
 *   byte 23 and the GUID at byte 28, every other byte behind the RecordHeader
 *   zero, the magic 0x2A724563 at 56.  Apart from the flags these are the bytes
 *   of bmqcrc_confirm_records_pack's DELETION records.
 * Outputs, each may be NULL: expired[n_records] (1 or 0); new_index[n_records]
 *   (j, or 0xFFFFFFFF); select_out[n_records] (1 exactly for MESSAGE records
 *   that are live and not expired: the next select for every other call);
 *   queue_expired[n_queues]; queue_front[n_queues] (front(q), 0xFFFFFFFF for
 *   none: the caller reads from it when that queue is next due).
 * Size only.  journal_dst == NULL with journal_dst_bytes == 0: everything is
 *   decided, nothing is stored (no output array either) and the result says
 *   what a real call would write.
 * All or nothing, decided on the device.  One violation anywhere refuses the
 *   call, and a refused call writes nothing.  The lowest kind wins and within
 *   it the lowest index (BMQCRC_EXPIRE_PACK_* below), whatever the order the
 *   device works in.  A synchronous call returns BMQCRC_EINVAL naming kind and
 *   index; after an asynchronous call bmqcrc_last_expire_records reports them.
 * What differs from the reference.
 *   - There is no e_NO_SC_QUORUM branch: receipts are not in the journal.
 *   - There is no `limit`: FileStore's own call passes none.
 *   - Records come out in journal order.  The reference visits queues in its
 *     storage map's order; inside a queue the order is the same.
 *   - No stats, no queue-engine callback, no virtual-storage bookkeeping.
 *   - Nothing is replicated: the output goes to bmqcrc_storage_event_pack.
 * Options.  Device pointers only: BMQCRC_F_DEVICE_PTRS is required,
 *   BMQCRC_F_ASYNC allowed; any other flag, ndevices > 1, a wrong struct_size or
 *   a non-zero reserved field; journal null; queue_keys or ttl_seconds null
 *   with n_queues != 0; journal_dst null with journal_dst_bytes != 0; journal,
 *   journal_dst, new_index, queue_expired or queue_front not 4-byte aligned,
 *   ttl_seconds not 8-byte aligned; journal_bytes != 60 n_records; n_records or
 *   n_queues >= 2^32; lease_id 0; first_seq 0 or first_seq + n_records above
 *   2^48 - 1; journal_dst or an output array meeting an input or one another is
 *   BMQCRC_EINVAL, answered on the host before the device lookup.
 *   n_records == 0 launches nothing, writes nothing (the per-queue arrays
 *   neither, and the table is not looked at) and reports zeros behind
 *   next_seq = first_seq.
 * *result (may be NULL) is written by a synchronous call only.
 * State.  As bmqcrc_confirm_records_pack: takes the workspace mutex of (device,
 *   stream); restores the caller's current device; allocates its own workspace
 *   on first use and when the call grows (14 bytes per record and 8 to 16 more
 *   for the hash, 8 per table entry and 8 to 16 more for its hash), which
 *   bmqcrc_reserve does not cover; is not meant to be captured into a hipGraph;
 *   is deterministic.  The shape prediction and the records of every other
 *   bmqcrc_last_* call are never touched. */
#define BMQCRC_EXPIRE_PACK_OK 0
#define BMQCRC_EXPIRE_PACK_RECORD_HEADER 1      /* BMQCRC_CONFIRM_PACK_RECORD_HEADER's conditions, on every
                                                   record of the run.  Index: the record */
#define BMQCRC_EXPIRE_PACK_DUPLICATE_MESSAGE 2  /* two selected MESSAGE records share a key.  Index: the
                                                   lowest record among all that share theirs */
#define BMQCRC_EXPIRE_PACK_QUEUE_KEY 3          /* a table entry whose key is all zero, or a key that stands
                                                   in the table twice.  Index: the entry; for a repeat the
                                                   lowest entry among all that share theirs */
#define BMQCRC_EXPIRE_PACK_DST_TOO_SMALL 4      /* index: the lowest MESSAGE record whose DELETION record
                                                   ends past journal_dst_bytes */

typedef struct bmqcrc_expire_pack {
    uint32_t struct_size, reserved;       /* sizeof, 0 */
    const void* journal;                  /* device, 4-byte aligned: n_records 60-byte records, the record run */
    uint64_t journal_bytes;               /* == 60 * n_records */
    uint64_t n_records;                   /* < 2^32 */
    const uint8_t* select;                /* device, n_records, may be NULL (every MESSAGE record) */
    const uint8_t* queue_keys;            /* device, 5 n_queues (may be NULL when n_queues is 0) */
    const uint64_t* ttl_seconds;          /* device, n_queues, 8-byte aligned (may be NULL likewise) */
    uint64_t n_queues;                    /* < 2^32 */
    uint64_t now;                         /* seconds from the epoch; every written record's timestamp */
    uint64_t first_seq;                   /* sequence number of the first record written, not 0 */
    uint32_t lease_id;                    /* primary lease id, not 0 */
    uint32_t reserved2;                   /* 0 */
    void* journal_dst;                    /* device, 4-byte aligned: the 60-byte records back to back;
                                             NULL (journal_dst_bytes 0): size only */
    uint64_t journal_dst_bytes;
    uint8_t* expired;                     /* device, n_records, may be NULL */
    uint32_t* new_index;                  /* device, n_records, may be NULL */
    uint8_t* select_out;                  /* device, n_records, may be NULL */
    uint32_t* queue_expired;              /* device, n_queues, may be NULL */
    uint32_t* queue_front;                /* device, n_queues, may be NULL */
} bmqcrc_expire_pack;

/* All fields zero before the first call on (device, stream); after a refused
 * call only n_records and the refused_* fields are set. */
typedef struct bmqcrc_expire_pack_result {
    uint64_t n_records;
    uint64_t n_live;                      /* live MESSAGE records, the expired ones among them */
    uint64_t n_expired;                   /* DELETION records written */
    uint64_t n_no_queue;                  /* live MESSAGE records without a table entry */
    uint64_t journal_bytes;               /* 60 n_expired */
    uint64_t next_seq;                    /* first_seq + n_expired */
    uint32_t refused_kind, reserved;
    uint64_t refused_index;               /* a record or a table entry, by kind */
} bmqcrc_expire_pack_result;

int bmqcrc_expire_records_pack(const bmqcrc_expire_pack* p, bmqcrc_expire_pack_result* result,
                               const bmqcrc_opts* opts);

/* ABI 2.20.  Result of the previous bmqcrc_expire_records_pack on (device,
 * stream); waits for it.  `result` may be NULL. */
int bmqcrc_last_expire_records(int device, void* stream, bmqcrc_expire_pack_result* result);

/* ABI 2.21.  What to deliver to whom: the messages of a device-resident
 * partition that each consumer (app) still has to see, listed ON THE DEVICE as
 * the records[], queue_ids[] and sub_ids[] bmqcrc_push_event_pack takes, in one
 * call.  In the reference this is mqbi::Storage::getIterator(appKey) --
 * FileBackedStorage::getIterator, VirtualStorageCatalog::begin and
 * VirtualStorageIterator::advance, which skips every message whose
 * appMessageView(ordinal) is not pending -- over the state that
 * FileBackedStorage::processMessageRecord, processConfirmRecord and
 * processDeletionRecord rebuild record by record after a restart.  This call
 * has no CRC in it: no payload byte is read.  It is here because it was the one
 * step between the device calls that still needed the journal on the host.
 *
 * The journal is the state, as in bmqcrc_confirm_records_pack and
 *   bmqcrc_expire_records_pack: the run (journal, journal_bytes == 60
 *   n_records), select and key = (GUID, queue key) mean what they mean there.
 * The consumer table has the shape of the reference's one storage per queue
 *   with its virtual storages by ordinal, in CSR form: queue q = 0 .. n_queues
 *   - 1 is queue_keys[5 q .. +5) and owns the apps app_first[q] ..
 *   app_first[q + 1] - 1; an app's ORDINAL is its position in that range; a
 *   queue has at most 32 apps, so that a message's per-app state is one word.
 *   App a = 0 .. n_apps - 1 is app_keys[5 a .. +5) (all zero: the null key),
 *   queue_ids[a] and sub_ids[a] (what bmqcrc_push_pack wants for this
 *   consumer; sub_ids may be NULL), from_record[a] (may be NULL: all 0; the
 *   delivery cursor, messages below it are not listed) and limit[a] (may be
 *   NULL: no limit; the consumer's remaining maxUnconfirmedMessages).
 * For a selected MESSAGE record m:
 *   - live(m): no DELETION record anywhere in the run has its key.
 *   - queue(m): the table's queue whose 5 bytes equal bytes 22..26 of m, or
 *     none.  A live message without a queue is never listed and is counted in
 *     n_no_queue.
 *   - confirmed(m, a): a is an app of queue(m) with a NON-NULL app key, and some
 *     CONFIRM record of the run has m's key and, in bytes 27..31, a's app key.
 *     Any reason counts, e_AUTO_CONFIRMED included, wherever the record stands
 *     in the run.  A CONFIRM record with a null app key marks nothing
 *     (processConfirmRecord's `if (!appKey.isNull())`).  A CONFIRM record whose
 *     message is found but whose app key no app of the queue has (or whose
 *     queue is not in the table) is counted in n_unknown_confirms and has no
 *     effect: the reference logs #STORAGE_INVALID_CONFIRM and ignores it.  A
 *     CONFIRM record whose key no selected MESSAGE record has is counted in
 *     n_not_found, whatever its app key.
 *   - pending(m, a): live(m), a is an app of queue(m), not confirmed(m, a) and
 *     m >= from_record[a].  An app with the null key therefore sees every live
 *     message of its queue: the reference's getIterator(k_NULL_KEY).
 *   - list(a): the pending records of a in journal order; listed(a): its first
 *     min(|list(a)|, limit[a]); next(a): the record at position limit[a] of
 *     list(a), or n_records when there is none -- the next call's
 *     from_record[a].
 * Outputs, grouped by app in table order and in journal order inside an app:
 *   records[list_cap], out_queue_ids[list_cap] and out_sub_ids[list_cap] (may
 *   be NULL, must be NULL when sub_ids is) hold listed(a) at [list_first[a],
 *   list_first[a + 1]), list_first[n_apps + 1] being the prefix of |listed(a)|.
 *   The three are exactly the arrays bmqcrc_push_event_pack takes.  list_first
 *   has event_first's type, for a caller that cuts one event per app: an EMPTY
 *   app repeats an entry, which event_first refuses, so such a caller drops the
 *   repeats first.  Per app, each may be NULL: app_pending[n_apps] (|list(a)|)
 *   and app_next[n_apps] (next(a)).  Per record, may be NULL:
 *   pending_mask[n_records], bit `ordinal` set when pending(m, a), 0 for every
 *   record that is not a live selected MESSAGE record with a queue.
 * Size only.  records == NULL with list_cap == 0: everything is decided,
 *   nothing is stored (no output array either) and the result says what a real
 *   call would write.
 * All or nothing, decided on the device.  One violation anywhere refuses the
 *   call, and a refused call writes nothing.  The lowest kind wins and within
 *   it the lowest index (BMQCRC_PENDING_LIST_* below), whatever the order the
 *   device works in.  A synchronous call returns BMQCRC_EINVAL naming kind and
 *   index; after an asynchronous call bmqcrc_last_pending_records reports them.
 * What differs from the reference.
 *   - Per-app PURGE records (a QueueOpType::e_PURGE with a non-null app key)
 *     are NOT honoured: the reference's form carries a start lease and sequence
 *     number, which the selection would have to learn first.  Whole-queue
 *     purges and queue deletions are `select`'s (bmqcrc_journal_select).  This
 *     is the first follow-up.
 *   - No RDA counters, no receipts (hasReceipt), no in-flight "pushing" state:
 *     the cursor and the limit are the caller's.
 *   - An app added after a message was stored is handled by the caller's
 *     from_record; in the reference this is d_defaultNonApplicableAppMessage.
 * Options.  Device pointers only: BMQCRC_F_DEVICE_PTRS is required,
 *   BMQCRC_F_ASYNC allowed; any other flag, ndevices > 1, a wrong struct_size or
 *   a non-zero reserved field; journal, app_first or (unless size-only)
 *   out_queue_ids or list_first null; queue_keys null with n_queues != 0;
 *   app_keys or queue_ids null with n_apps != 0; records null with list_cap !=
 *   0; out_sub_ids without sub_ids; journal or a uint32 / int32 array not 4-byte
 *   aligned, app_first or list_first not 8-byte aligned (queue_keys, app_keys
 *   and select may stand at any byte); journal_bytes != 60 n_records;
 *   n_records, n_queues or n_apps >= 2^32; an output meeting an input or
 *   another output is BMQCRC_EINVAL, answered on the host before the device
 *   lookup.  n_records == 0 launches nothing, writes nothing (list_first
 *   neither, and the table is not looked at) and reports zeros.
 * *result (may be NULL) is written by a synchronous call only.
 * State.  As bmqcrc_expire_records_pack: takes the workspace mutex of (device,
 *   stream); restores the caller's current device; allocates its own workspace
 *   on first use and when the call grows (22 bytes per record and 8 to 16 more
 *   for the hash, 8 to 16 per queue, 16 per app, 16 per pair (app, message)
 *   that is pending), which bmqcrc_reserve does not cover; is not meant to be
 *   captured into a hipGraph; is deterministic.  The pairs are counted on the
 *   device and that ONE WORD is read by the host, in the middle of the call, to
 *   size the sort's buffers: the call therefore waits for its first four
 *   kernels whether or not BMQCRC_F_ASYNC is set, and BMQCRC_F_ASYNC leaves the
 *   sort and the stores in flight.  (Sizing by the bound of 32 pairs a message
 *   would need no wait and 512 bytes a record.)  The shape prediction and the
 *   records of every other bmqcrc_last_* call are never touched. */
#define BMQCRC_PENDING_LIST_OK 0
#define BMQCRC_PENDING_LIST_RECORD_HEADER 1      /* BMQCRC_CONFIRM_PACK_RECORD_HEADER's conditions, on
                                                    every record of the run.  Index: the record */
#define BMQCRC_PENDING_LIST_DUPLICATE_MESSAGE 2  /* two selected MESSAGE records share a key.  Index:
                                                    the lowest record among all that share theirs */
#define BMQCRC_PENDING_LIST_QUEUE_KEY 3          /* an all-zero queue key, or one that stands in the
                                                    table twice.  Index: the lowest such queue */
#define BMQCRC_PENDING_LIST_APP_FIRST 4          /* app_first[0] != 0 (index 0); app_first[q] >
                                                    app_first[q + 1] or more than 32 apps (index q);
                                                    app_first[n_queues] != n_apps (index n_queues).
                                                    The lowest such index */
#define BMQCRC_PENDING_LIST_APP_KEY 5            /* two apps of one queue share an app key (the null
                                                    key may stand once too).  Index: the lowest app
                                                    among them */
#define BMQCRC_PENDING_LIST_FROM_RECORD 6        /* from_record[a] > n_records.  Index: the app */
#define BMQCRC_PENDING_LIST_LIST_TOO_SMALL 7     /* index: the lowest app whose listed entries end past
                                                    list_cap; n_apps when the sum of |list(a)| is 2^32
                                                    or more (a size-only call raises only this) */

typedef struct bmqcrc_pending_list {
    uint32_t struct_size, reserved;       /* sizeof, 0 */
    const void* journal;                  /* device, 4-byte aligned: n_records 60-byte records, the record run */
    uint64_t journal_bytes;               /* == 60 * n_records */
    uint64_t n_records;                   /* < 2^32 */
    const uint8_t* select;                /* device, n_records, may be NULL (every MESSAGE record) */
    const uint8_t* queue_keys;            /* device, 5 n_queues (may be NULL when n_queues is 0) */
    const uint64_t* app_first;            /* device, n_queues + 1, 8-byte aligned */
    uint64_t n_queues;                    /* < 2^32 */
    const uint8_t* app_keys;              /* device, 5 n_apps (may be NULL when n_apps is 0) */
    const int32_t* queue_ids;             /* device, n_apps (may be NULL likewise) */
    const uint32_t* sub_ids;              /* device, n_apps, may be NULL */
    const uint32_t* from_record;          /* device, n_apps, may be NULL (all 0) */
    const uint32_t* limit;                /* device, n_apps, may be NULL (no limit) */
    uint64_t n_apps;                      /* < 2^32 */
    uint32_t* records;                    /* device, list_cap; NULL (list_cap 0): size only */
    int32_t* out_queue_ids;               /* device, list_cap */
    uint32_t* out_sub_ids;                /* device, list_cap, may be NULL; NULL when sub_ids is */
    uint64_t list_cap;                    /* entries */
    uint64_t* list_first;                 /* device, n_apps + 1, 8-byte aligned */
    uint32_t* app_pending;                /* device, n_apps, may be NULL */
    uint32_t* app_next;                   /* device, n_apps, may be NULL */
    uint32_t* pending_mask;               /* device, n_records, may be NULL */
} bmqcrc_pending_list;

/* All fields zero before the first call on (device, stream); after a refused
 * call only n_records and the refused_* fields are set. */
typedef struct bmqcrc_pending_list_result {
    uint64_t n_records;
    uint64_t n_live;                      /* live MESSAGE records */
    uint64_t n_no_queue;                  /* ... of them without a queue in the table */
    uint64_t n_pending;                   /* the sum of |list(a)| */
    uint64_t n_listed;                    /* entries written (or, size-only, that a real call writes) */
    uint64_t n_unknown_confirms;          /* CONFIRM records whose app key no app of the queue has */
    uint64_t n_not_found;                 /* CONFIRM records without a selected MESSAGE record */
    uint32_t refused_kind, reserved;
    uint64_t refused_index;               /* a record, a queue or an app, by kind */
} bmqcrc_pending_list_result;

int bmqcrc_pending_records_list(const bmqcrc_pending_list* p, bmqcrc_pending_list_result* result,
                                const bmqcrc_opts* opts);

/* ABI 2.21.  Result of the previous bmqcrc_pending_records_list on (device,
 * stream); waits for it.  `result` may be NULL. */
int bmqcrc_last_pending_records(int device, void* stream, bmqcrc_pending_list_result* result);

/* ---- cluster state ledger (mqbc_clusterstateledgerprotocol.h:76,272) ------ */

/* mqbc::ClusterStateLedgerUtilRc values (mqbc_clusterstateledgerutil.h:65-124)
 * and the one mqbsi::LogOpResult a log walk can return (mqbsi_log.h:138). */
#define BMQCRC_CSL_SUCCESS 0
#define BMQCRC_CSL_INVALID_PROTOCOL_VERSION (-5)
#define BMQCRC_CSL_INVALID_LOG_ID (-6)
#define BMQCRC_CSL_INVALID_HEADER_WORDS (-7)
#define BMQCRC_CSL_INVALID_CHECKSUM (-10)
#define BMQCRC_CSL_RECORD_ALIAS_FAILURE (-13)
#define BMQCRC_CSL_REACHED_END_OF_LOG (-15)

/* Walk a ledger log like validateLog without the CRC check: validate the
 * ClusterStateFileHeader (against the 5-byte expected_log_id unless NULL),
 * then records while a whole ClusterStateRecordHeader fits; the walk stops
 * cleanly at the first invalid record header.  For record i: rec_off, and
 * rec_len = header + advisory + padding (the CRC'd bytes), crc = the trailing
 * big-endian CRC32C.  *walk_rc = the validateLog code the walk alone yields
 * (0, a file-header code, or REACHED_END_OF_LOG for a record running past
 * the end); *end_offset = where a clean walk stopped. */
int64_t bmqcrc_csl_scan(const void* log, uint64_t len, const uint8_t* expected_log_id,
                        uint64_t* rec_off, uint32_t* rec_len, uint32_t* crc, uint64_t cap,
                        int* walk_rc, uint64_t* end_offset);

/* ClusterStateLedgerUtil::validateLog with every record CRC checked in one
 * batch.  *csl_rc receives exactly the reference's result: 0 with *offset =
 * end of the valid records, INVALID_CHECKSUM for the first (lowest offset)
 * corrupt record (its offset in *bad_record_off if non-NULL), or the walk's
 * code.  The return value is a BMQCRC_E* status of the call itself. */
int bmqcrc_csl_validate(const void* log, uint64_t len, const uint8_t* expected_log_id,
                        int* csl_rc, uint64_t* offset, uint64_t* bad_record_off,
                        const bmqcrc_opts* opts);

#ifdef __cplusplus
}  /* extern "C" */

#include <vector>

/* ---- C++ spellings at the reference call sites -------------------------- */
/* The reference's calls have no error channel (bmqp_crc32c.h:240-243), so
 * these spellings never surface a GPU failure: when the batched MI355X call
 * fails for want of a GPU (BMQCRC_ENODEV, ENOMEM, EIO) they redo the same
 * walk and CRC every message on the host with the library's own SSE4.2 code
 * (bmqcrc_crc32c), bit-exact.  Format errors (BMQCRC_EINVAL) are returned.
 * Every fallback is recorded (bmqcrc_host_fallbacks, bmqcrc.h); a fault (EIO)
 * is also reported on stderr once.  The C-ABI batch entry points above stay
 * GPU-only. */
namespace BloombergLP {
namespace bmqcrc_detail {
inline bool gpuFailure(int64_t rc)
{
    if (rc == BMQCRC_ENODEV || rc == BMQCRC_ENOMEM || rc == BMQCRC_EIO) {
        bmqcrc_note_host_fallback((int32_t)rc);
        return true;
    }
    return false;
}
inline uint32_t be32(const uint8_t* p)
{
    return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
}
}  // close namespace bmqcrc_detail

namespace bmqp {
/// Batched counterpart of the CRC step of `PutEventBuilder::packMessage`
/// (bmqp_puteventbuilder.cpp:302-320) and `PutMessageIterator` (:678), over a
/// flattened PUT event.
struct PutEventCrc32c {
    static int64_t fillAll(void* event, uint64_t len, const bmqcrc_opts* opts = 0)
    {
        const int64_t rc = bmqcrc_put_event_fill_crcs(event, len, opts);
        if (!bmqcrc_detail::gpuFailure(rc)) {
            return rc;
        }
        const int64_t n = bmqcrc_put_event_scan(event, len, 0, 0, 0, 0);
        if (n <= 0) {
            return n;
        }
        std::vector<uint64_t> off(n), pos(n);
        std::vector<uint32_t> ln(n);
        bmqcrc_put_event_scan(event, len, off.data(), ln.data(), pos.data(), n);
        uint8_t* ev = static_cast<uint8_t*>(event);
        for (int64_t i = 0; i < n; ++i) {
            const uint32_t c = bmqcrc_crc32c(ev + off[i], ln[i], 0);
            ev[pos[i]] = (uint8_t)(c >> 24);
            ev[pos[i] + 1] = (uint8_t)(c >> 16);
            ev[pos[i] + 2] = (uint8_t)(c >> 8);
            ev[pos[i] + 3] = (uint8_t)c;
        }
        return n;
    }
    static int verifyAll(const void* event, uint64_t len, uint64_t* numMessages,
                         uint64_t* numBad, uint64_t* badIndices = 0, uint64_t badCap = 0,
                         const bmqcrc_opts* opts = 0)
    {
        const int rc = bmqcrc_put_event_verify(event, len, numMessages, numBad, badIndices,
                                               badCap, opts);
        if (!bmqcrc_detail::gpuFailure(rc)) {
            return rc;
        }
        const int64_t n = bmqcrc_put_event_scan(event, len, 0, 0, 0, 0);
        if (n < 0) {
            return (int)n;
        }
        std::vector<uint64_t> off(n), pos(n);
        std::vector<uint32_t> ln(n);
        bmqcrc_put_event_scan(event, len, off.data(), ln.data(), pos.data(), n);
        const uint8_t* ev = static_cast<const uint8_t*>(event);
        uint64_t bad = 0;
        for (int64_t i = 0; i < n; ++i) {
            if (bmqcrc_crc32c(ev + off[i], ln[i], 0) != bmqcrc_detail::be32(ev + pos[i])) {
                if (bad < badCap) {
                    badIndices[bad] = (uint64_t)i;
                }
                ++bad;
            }
        }
        *numMessages = (uint64_t)n;
        *numBad = bad;
        return 0;
    }
};
}  // close namespace bmqp

namespace mqbs {
/// Batched CRC check of `FileStore::recoverMessages` (mqbs_filestore.cpp:2603),
/// over the same records the reference CRCs (see bmqcrc_recover_verify).
struct FileStoreCrc32c {
    static int verifyRecovery(const void* journal, uint64_t journalLen, const void* data,
                              uint64_t dataLen, int* recoveryRc, uint64_t* numMessages,
                              uint64_t* numBad, uint64_t* badRecordOffsets = 0,
                              uint64_t badCap = 0, const bmqcrc_recovery_cfg* cfg = 0,
                              const bmqcrc_opts* opts = 0, uint64_t* errorRecordOffset = 0)
    {
        const int rc = bmqcrc_recover_verify(journal, journalLen, data, dataLen, cfg, recoveryRc,
                                             errorRecordOffset, numMessages, numBad,
                                             badRecordOffsets, badCap, opts);
        if (!bmqcrc_detail::gpuFailure(rc)) {
            return rc;
        }
        const int64_t n = bmqcrc_journal_scan(journal, journalLen, data, dataLen, cfg,
                                              recoveryRc, errorRecordOffset, 0, 0, 0, 0, 0);
        if (n < 0) {
            return (int)n;
        }
        std::vector<uint64_t> rec(n), off(n);
        std::vector<uint32_t> ln(n), crc(n);
        bmqcrc_journal_scan(journal, journalLen, data, dataLen, cfg, recoveryRc,
                            errorRecordOffset, rec.data(), off.data(), ln.data(), crc.data(), n);
        const uint8_t* d = static_cast<const uint8_t*>(data);
        uint64_t bad = 0;
        for (int64_t i = 0; i < n; ++i) {
            if (bmqcrc_crc32c(d + off[i], ln[i], 0) != crc[i]) {
                if (bad < badCap) {
                    badRecordOffsets[bad] = rec[i];
                }
                ++bad;
            }
        }
        *numMessages = (uint64_t)n;
        *numBad = bad;
        return 0;
    }
};
}  // close namespace mqbs

namespace mqbc {
/// `ClusterStateLedgerUtil::validateLog` (mqbc_clusterstateledgerutil.cpp:248)
/// over a mapped log: returns the reference's rc, sets `*offset` on success.
struct ClusterStateLedgerCrc32c {
    static int validateLog(uint64_t* offset, const void* log, uint64_t len,
                           const uint8_t* expectedLogId = 0, const bmqcrc_opts* opts = 0)
    {
        int cslRc = 0;
        const int rc = bmqcrc_csl_validate(log, len, expectedLogId, &cslRc, offset, 0, opts);
        if (!bmqcrc_detail::gpuFailure(rc)) {
            return rc ? rc * 1000 : cslRc;
        }
        int walkRc = 0;
        uint64_t end = 0;
        const int64_t n = bmqcrc_csl_scan(log, len, expectedLogId, 0, 0, 0, 0, &walkRc, &end);
        if (n < 0) {
            return (int)n * 1000;
        }
        std::vector<uint64_t> off(n);
        std::vector<uint32_t> ln(n), crc(n);
        bmqcrc_csl_scan(log, len, expectedLogId, off.data(), ln.data(), crc.data(), n, &walkRc,
                        &end);
        const uint8_t* a = static_cast<const uint8_t*>(log);
        for (int64_t i = 0; i < n; ++i) {  // the first corrupt record in log order
            if (bmqcrc_crc32c(a + off[i], ln[i], 0) != crc[i]) {
                return BMQCRC_CSL_INVALID_CHECKSUM;
            }
        }
        if (walkRc == 0) {
            *offset = end;
        }
        return walkRc;
    }
};
}  // close namespace mqbc
}  // close enterprise namespace
#endif /* __cplusplus */

#endif /* BMQCRC_PROTOCOL_H */
