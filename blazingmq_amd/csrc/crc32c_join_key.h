// crc32c_join_key.h -- the order-free join of journal records by GUID and
// queue key: the key, its hash and the open-addressing table of MESSAGE records
// the device calls build and probe (DESIGN.md sections 20 to 23).  Device
// only, in the anonymous namespace like the units' own code.
//
//   JoinKey, join_key, same_key, key_hash,      crc32c_rollover.hip,
//   JoinTable, join_insert, join_find           crc32c_confirm_records.hip,
//                                               crc32c_expire_records.hip,
//                                               crc32c_pending_list.hip
//   QueueTable, table_key, table_key_of,        crc32c_pending_list.hip
//   table_insert, table_find                    (crc32c_expire_records.hip keeps
//                                               its own queue_* over ExpArgs, whose
//                                               text tests/expire_collisions.py
//                                               mirrors; these are the same walk)
//
// A slot holds record + 1 of a MESSAGE record of the run (0: empty), so the
// table stores no key: a probe compares with the record's own bytes, read by a
// record index below the run's n only.  The table has a power of two of slots,
// at least twice the records, zeroed before the call: a walk ends at an empty
// slot.  Nothing is ever removed, so a key that is in the table is met by
// every later walk for it before that walk meets an empty slot.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bmqcrc_internal.h"

namespace bmqcrc {
namespace {

// dwords of a record: the GUID of a MESSAGE record (bytes 36..51), of a
// CONFIRM record (32..47) and of a DELETION record (28..43); the queue key of
// the first two lies in bytes 22..26, a DELETION record's in 23..27
constexpr uint32_t kMsgGuidDword = 9, kCfmGuidDword = 8, kDelGuidDword = 7;

// What the join compares: the GUID and the queue key's five bytes, the first
// two in q0 and the other three in q1 as they lie in memory.
struct JoinKey {
    uint32_t g[4], q0, q1;
};

// Of a MESSAGE or CONFIRM record's dwords.
__device__ __forceinline__ JoinKey join_key(const uint32_t* d, uint32_t guid_dword)
{
    JoinKey k;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        k.g[j] = d[guid_dword + j];
    }
    k.q0 = d[5] >> 16;          // bytes 22, 23
    k.q1 = d[6] & 0x00FFFFFFu;  // bytes 24..26
    return k;
}

// Of a DELETION record's dwords: its queue key starts one byte later.
__device__ __forceinline__ JoinKey join_key_deletion(const uint32_t* d)
{
    JoinKey k;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        k.g[j] = d[kDelGuidDword + j];
    }
    k.q0 = (d[5] >> 24) | ((d[6] & 0xFFu) << 8);  // bytes 23, 24
    k.q1 = d[6] >> 8;                             // bytes 25..27
    return k;
}

// Of a GUID's 16 and a queue key's 5 bytes, at any alignment.
__device__ __forceinline__ JoinKey join_key_bytes(const uint8_t* guid, const uint8_t* qk)
{
    JoinKey k;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        k.g[j] = (uint32_t)guid[4 * j] | ((uint32_t)guid[4 * j + 1] << 8) |
                 ((uint32_t)guid[4 * j + 2] << 16) | ((uint32_t)guid[4 * j + 3] << 24);
    }
    k.q0 = (uint32_t)qk[0] | ((uint32_t)qk[1] << 8);
    k.q1 = (uint32_t)qk[2] | ((uint32_t)qk[3] << 8) | ((uint32_t)qk[4] << 16);
    return k;
}

__device__ __forceinline__ bool same_key(const JoinKey& x, const JoinKey& y)
{
    return x.g[0] == y.g[0] && x.g[1] == y.g[1] && x.g[2] == y.g[2] && x.g[3] == y.g[3] &&
           x.q0 == y.q0 && x.q1 == y.q1;
}

// Every byte of the key reaches every bit of the slot: a multiply and a fold
// per word, and a last avalanche.
__device__ __forceinline__ uint32_t key_hash(const JoinKey& k)
{
    uint32_t h = 0x9E3779B9u;
    const uint32_t w[6] = {k.g[0], k.g[1], k.g[2], k.g[3], k.q0, k.q1};
#pragma unroll
    for (uint32_t j = 0; j < 6; ++j) {
        h = (h ^ w[j]) * 0x85EBCA6Bu;
        h ^= h >> 15;
    }
    h *= 0xC2B2AE35u;
    return h ^ (h >> 16);
}

struct JoinTable {
    uint32_t* slot;           // slots words, zeroed before the call
    uint64_t slots;           // a power of two, at least twice the run's records
    const uint32_t* journal;  // the run: a slot's record is read from here
};

// MESSAGE record r, whose key is k, into the table unless its key is there
// already: returns 0 when r took a slot, otherwise record + 1 of the MESSAGE
// record that holds the key (a chain never grows with repeats of a key).
__device__ __forceinline__ uint32_t join_insert(const JoinTable& t, const JoinKey& k, uint64_t r)
{
    const uint64_t mask = t.slots - 1;
    uint64_t s = key_hash(k) & mask;
    for (uint64_t step = 0; step < t.slots; ++step, s = (s + 1) & mask) {
        const uint32_t cur = atomicCAS(&t.slot[s], 0u, (uint32_t)r + 1u);
        if (cur == 0) {
            return 0;
        }
        if (same_key(k, join_key(t.journal + (uint64_t)kJournalRecordDwords * (cur - 1u),
                                 kMsgGuidDword))) {
            return cur;
        }
    }
    return 0;
}

// Record + 1 of the MESSAGE record in the table that has this key, 0 when
// none has.  For a table that is whole: every insert has ended.
__device__ __forceinline__ uint32_t join_find(const JoinTable& t, const JoinKey& k)
{
    const uint64_t mask = t.slots - 1;
    uint64_t s = key_hash(k) & mask;
    for (uint64_t step = 0; step < t.slots; ++step, s = (s + 1) & mask) {
        const uint32_t cur = t.slot[s];
        if (cur == 0) {
            return 0;
        }
        if (same_key(k, join_key(t.journal + (uint64_t)kJournalRecordDwords * (cur - 1u),
                                 kMsgGuidDword))) {
            return cur;
        }
    }
    return 0;
}

// ---- a queue table's hash: a slot holds entry + 1 (0: empty) and no key, a
// probe compares with the table's own 5-byte keys, read by an entry below the
// table's length only.  A power of two of slots, at least twice the entries,
// zeroed before the call; nothing is ever removed.  A queue key is hashed as a
// JoinKey under the null GUID, so a record's (q0, q1) probes it as they are.

struct QueueTable {
    uint32_t* slot;       // slots words, zeroed before the call
    uint64_t slots;       // a power of two, at least twice the entries (0: an empty table)
    const uint8_t* keys;  // the table: 5 bytes an entry, at any alignment
};

// A queue key as the join holds one (q0, q1), under the null GUID.
__device__ __forceinline__ JoinKey table_key(uint32_t q0, uint32_t q1)
{
    return {{0u, 0u, 0u, 0u}, q0, q1};
}

// Entry e's.
__device__ __forceinline__ JoinKey table_key_of(const QueueTable& t, uint64_t e)
{
    const uint8_t null_guid[16] = {0};
    return join_key_bytes(null_guid, t.keys + 5 * e);
}

// Entry e, whose key is k, into the table unless its key is there already:
// returns 0 when e took a slot, otherwise entry + 1 of the one that holds it.
__device__ __forceinline__ uint32_t table_insert(const QueueTable& t, const JoinKey& k, uint64_t e)
{
    const uint64_t mask = t.slots - 1;
    uint64_t s = key_hash(k) & mask;
    for (uint64_t step = 0; step < t.slots; ++step, s = (s + 1) & mask) {
        const uint32_t cur = atomicCAS(&t.slot[s], 0u, (uint32_t)e + 1u);
        if (cur == 0) {
            return 0;
        }
        if (same_key(k, table_key_of(t, cur - 1u))) {
            return cur;
        }
    }
    return 0;
}

// Entry + 1 of the one that has this key, 0 when none has.  For a table that
// is whole (or has no slot at all: no entry).
__device__ __forceinline__ uint32_t table_find(const QueueTable& t, const JoinKey& k)
{
    const uint64_t mask = t.slots - 1;
    uint64_t s = key_hash(k) & mask;
    for (uint64_t step = 0; step < t.slots; ++step, s = (s + 1) & mask) {
        const uint32_t cur = t.slot[s];
        if (cur == 0) {
            return 0;
        }
        if (same_key(k, table_key_of(t, cur - 1u))) {
            return cur;
        }
    }
    return 0;
}

}  // namespace
}  // namespace bmqcrc
