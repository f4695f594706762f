"""Hand-worked inputs of bmqcrc_expire_records_pack (ABI 2.20) with the answers
written out, shared by tests/test_expire_records_model.py (the model alone) and
tests/test_gpu_expire_records.py (the device against the model).  No test in
here.  Every run is the records of a journal, without the file's header."""
import collections

import numpy as np

from blazingmq_amd import storage as S
import expire_records_model as M

JH = S.PartitionWriter.JOURNAL_HEADER
KEY_A, KEY_B, KEY_C = b"\x26\xda\xcd\xc9\x74", b"\x26\xda\xcd\xc9\x75", b"\x00\x00\x00\x00\x01"
LEASE = 3
NOW = 1000
G = [bytes([0x40 + i]) * 16 for i in range(8)]

Case = collections.namedtuple(
    "Case", "run table kw expired select_out queue_front queue_expired n_live n_no_queue")
Refused = collections.namedtuple("Refused", "name run table kw kind index")


def table(entries):
    """(queue_keys, ttl_seconds) of (key, ttl) pairs."""
    keys = np.frombuffer(b"".join(k for k, _ in entries), np.uint8).copy()
    return keys, np.array([t for _, t in entries], np.uint64)


def _run(w):
    run = w.files()[0][JH:].copy()
    run.setflags(write=False)
    return run


def ten_messages():
    """(run, next sequence number) of the reference's GARBAGE COLLECT test: ten
    messages of queue KEY_A with timestamps 1..10."""
    w = S.PartitionWriter(lease_id=LEASE)
    for i in range(10):
        w.message(b"data", KEY_A, timestamp=i + 1)
    return _run(w), w.seq + 1


def _case(w, entries, expired, select_out, queue_front, queue_expired, n_live, n_no_queue,
          **kw):
    kw = dict(dict(now=NOW, lease_id=LEASE, first_seq=w.seq + 1), **kw)
    return Case(_run(w), table(entries), kw, expired, select_out, queue_front, queue_expired,
                n_live, n_no_queue)


def a_future_dated_head_expires():
    """now - 2000 wraps to nearly 2^64, far above any TTL: the head goes, and
    the walk ends at the message behind it, 50 seconds old."""
    w = S.PartitionWriter(lease_id=LEASE)
    w.message(b"", KEY_A, guid=G[0], timestamp=2000)
    w.message(b"", KEY_A, guid=G[1], timestamp=950)
    w.message(b"", KEY_A, guid=G[2], timestamp=3000)    # future-dated too, but shielded
    return _case(w, [(KEY_A, 100)], [0], [1, 2], [1], [1], 3, 0)


def a_young_message_shields_the_old_one_behind_it():
    w = S.PartitionWriter(lease_id=LEASE)
    w.message(b"", KEY_A, guid=G[0], timestamp=950)
    w.message(b"", KEY_A, guid=G[1], timestamp=100)
    return _case(w, [(KEY_A, 100)], [], [0, 1], [0], [0], 2, 0)


def one_guid_under_two_queue_keys():
    """The same GUID in queue A (TTL 10) and queue B (TTL 1,000), both 100
    seconds old: two messages, of which A's expires.  Between them a message of
    A that is exactly TTL seconds old: `<=`, it has not expired."""
    w = S.PartitionWriter(lease_id=LEASE)
    w.message(b"", KEY_A, guid=G[0], timestamp=900)
    w.message(b"", KEY_B, guid=G[0], timestamp=900)
    w.message(b"", KEY_A, guid=G[1], timestamp=990)
    return _case(w, [(KEY_A, 10), (KEY_B, 1000)], [0], [1, 2], [2, 1], [1, 0], 3, 0)


def a_message_a_deletion_record_names():
    """Record 0 deletes the message of record 2 (a DELETION anywhere in the run
    counts), record 4 names a GUID of queue A under queue B's key: nobody."""
    w = S.PartitionWriter(lease_id=LEASE)
    w.deletion(G[1], KEY_A)
    w.message(b"", KEY_A, guid=G[0], timestamp=100)
    w.message(b"", KEY_A, guid=G[1], timestamp=100)
    w.message(b"", KEY_A, guid=G[2], timestamp=100)
    w.deletion(G[2], KEY_B)
    return _case(w, [(KEY_A, 100)], [1, 3], [], [M.NONE], [2], 2, 0)


def a_deselected_message_neither_expires_nor_shields():
    w = S.PartitionWriter(lease_id=LEASE)
    w.message(b"", KEY_A, guid=G[0], timestamp=990)     # young, but not selected
    w.message(b"", KEY_A, guid=G[1], timestamp=100)
    w.message(b"", KEY_A, guid=G[2], timestamp=100)     # old, but not selected
    w.message(b"", KEY_A, guid=G[3], timestamp=100)
    return _case(w, [(KEY_A, 100)], [1, 3], [], [M.NONE], [2], 2, 0,
                 select=np.array([0, 1, 0, 1], np.uint8))


def a_queue_absent_from_the_table():
    w = S.PartitionWriter(lease_id=LEASE)
    w.queue_op(S.OP_CREATION, KEY_C)
    w.message(b"", KEY_A, guid=G[0], timestamp=100)
    w.message(b"", KEY_C, guid=G[1], timestamp=100)
    w.sync_point()
    return _case(w, [(KEY_B, 0), (KEY_A, 100)], [1], [2], [M.NONE, M.NONE], [0, 1], 2, 1)


def the_longest_ttl_never_expires():
    """TTL 2^64 - 1: no difference exceeds it, whatever the timestamp; TTL 0
    beside it: only a message of this very second stays."""
    w = S.PartitionWriter(lease_id=LEASE)
    w.message(b"", KEY_A, guid=G[0], timestamp=2000)
    w.message(b"", KEY_A, guid=G[1], timestamp=0)
    w.message(b"", KEY_B, guid=G[2], timestamp=999)
    w.message(b"", KEY_B, guid=G[3], timestamp=1000)
    return _case(w, [(KEY_A, (1 << 64) - 1), (KEY_B, 0)], [2], [0, 1, 3], [0, 3], [0, 1], 4, 0)


HAND_WORKED = [a_future_dated_head_expires, a_young_message_shields_the_old_one_behind_it,
               one_guid_under_two_queue_keys, a_message_a_deletion_record_names,
               a_deselected_message_neither_expires_nor_shields, a_queue_absent_from_the_table,
               the_longest_ttl_never_expires]


# ---- one case per refusal condition ----------------------------------------------

def _old_messages(n=6):
    """(writer of n messages of queue A, all long expired at NOW, a CREATION
    record in front: the messages are records 1..n)."""
    w = S.PartitionWriter(lease_id=LEASE)
    w.queue_op(S.OP_CREATION, KEY_A)
    for i in range(n):
        w.message(b"", KEY_A, guid=G[i], timestamp=10 + i)
    return w


def refused():
    w = _old_messages()
    run, seq = _run(w), w.seq + 1
    kw = dict(now=NOW, lease_id=LEASE, first_seq=seq, journal_dst_bytes=360)
    good = table([(KEY_B, 5), (KEY_A, 100)])
    out = []

    def add(name, kind, index, run=run, tbl=good, **more):
        out.append(Refused(name, run, tbl, dict(kw, **more), kind, index))

    def edited(at, value, record):
        bad = np.array(run)
        bad[60 * record + at] = value
        return bad
    add("type_0", M.RECORD_HEADER, 2, run=edited(0, 0x00, 2))
    add("type_6", M.RECORD_HEADER, 6, run=edited(0, 0x60, 6))
    add("lease_0", M.RECORD_HEADER, 3, run=edited(11, 0, 3))
    add("seq_0", M.RECORD_HEADER, 4, run=edited(7, 0, 4))
    add("magic", M.RECORD_HEADER, 6, run=edited(59, 0x64, 6))
    add("queue_op_type_5", M.RECORD_HEADER, 0, run=edited(35, 5, 0))
    two = np.array(run)
    two[60 * 5 + 56], two[60 * 1 + 56] = 0, 0
    add("two_bad_headers_name_the_lower", M.RECORD_HEADER, 1, run=two)
    # record 5 a second MESSAGE record of record 2's key; record 6 of record 3's
    twin = np.array(run).reshape(-1, 60)
    twin[5, 20:56] = twin[2, 20:56]
    add("duplicate_message", M.DUPLICATE_MESSAGE, 2, run=twin.reshape(-1))
    twins = twin.copy()
    twins[6, 20:56] = twins[3, 20:56]
    add("two_duplicates_name_the_lowest", M.DUPLICATE_MESSAGE, 2, run=twins.reshape(-1))
    add("a_deselected_twin_is_no_duplicate_but_the_destination_is_short", M.DST_TOO_SMALL, 3,
        run=twin.reshape(-1), select=np.array([1, 1, 1, 1, 1, 0, 1], np.uint8),
        journal_dst_bytes=179)
    add("null_queue_key_in_the_last_entry", M.QUEUE_KEY, 2,
        tbl=table([(KEY_B, 5), (KEY_A, 100), (bytes(5), 7)]))
    add("a_queue_key_twice", M.QUEUE_KEY, 1,
        tbl=table([(KEY_B, 5), (KEY_A, 100), (KEY_C, 7), (KEY_A, 100)]))
    add("a_queue_key_three_times_and_a_null_key_above", M.QUEUE_KEY, 0,
        tbl=table([(KEY_C, 5), (KEY_A, 100), (KEY_C, 7), (bytes(5), 1), (KEY_C, 9)]))
    add("one_byte_short", M.DST_TOO_SMALL, 6, journal_dst_bytes=359)
    add("room_for_two", M.DST_TOO_SMALL, 3, journal_dst_bytes=120)
    add("no_room_at_all", M.DST_TOO_SMALL, 1, journal_dst_bytes=0)
    add("a_bad_header_above_a_null_queue_key", M.RECORD_HEADER, 6, run=edited(59, 0x64, 6),
        tbl=table([(bytes(5), 7)]))
    add("a_duplicate_above_a_short_destination", M.DUPLICATE_MESSAGE, 2, run=twin.reshape(-1),
        journal_dst_bytes=60)
    add("a_queue_key_twice_above_a_short_destination", M.QUEUE_KEY, 0,
        tbl=table([(KEY_A, 100), (KEY_A, 100)]), journal_dst_bytes=60)
    return out
