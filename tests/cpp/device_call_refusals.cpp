// device_call_refusals.cpp -- the refusals of the five struct-taking device
// calls (PUT pack, records pack, PUT unpack, records unpack, journal select)
// that answer before the device lookup: struct_size, reserved, the options,
// and the unpackers' output-overlaps-input table, with their texts and their
// order.  Needs no GPU and dereferences none of the pointers it hands over.
//
//   device_call_refusals        prints PASS, exit status 0
//
// blazingmq_amd/build.py links it against the product library
// (tests/test_cpu_path.py runs that).  To run the host runtime under the
// sanitizers, build a second copy of the library's sources with
//   hipcc -O1 -g -std=c++17 -Iinclude -fsanitize=address,undefined     (*.cpp)
//   hipcc ... -x hip --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined  (*.hip)
// into one program together with this file, and run it on a CPU machine.
#include "bmqcrc.h"
#include "bmqcrc_protocol.h"

#include <stdio.h>
#include <string.h>

#include <string>

static int g_fail = 0;

static void expect(int line, int rc, const std::string& want)
{
    const char* got = bmqcrc_last_error();
    if (rc != BMQCRC_EINVAL || want != (got ? got : "")) {
        fprintf(stderr, "line %d: rc %d, \"%s\"\n   wanted -22, \"%s\"\n", line, rc, got ? got : "",
                want.c_str());
        ++g_fail;
    }
}
#define EXPECT(call, text) expect(__LINE__, (call), (text))

static bmqcrc_opts options(uint32_t flags)
{
    bmqcrc_opts o;
    memset(&o, 0, sizeof(o));
    o.struct_size = sizeof(o);
    o.device = -1;
    o.flags = flags;
    return o;
}

// The preamble of one call: P its struct, `name` the struct's, `call` the entry point's.
template <class P, class Call>
static void preamble(const char* name, const char* call, Call fn,
                     const char* reserved_text = ".reserved must be 0")
{
    const std::string n = name, size_text = n + ".struct_size must be sizeof(" + n + ")";
    const bmqcrc_opts good = options(BMQCRC_F_DEVICE_PTRS), plan = options(BMQCRC_F_PLAN),
                      host = options(0);
    P p;
    memset(&p, 0, sizeof(p));
    EXPECT(fn(nullptr, &good), size_text);
    EXPECT(fn(&p, &good), size_text);  // struct_size 0
    p.struct_size = sizeof(p) + 8;
    p.reserved = 1;
    EXPECT(fn(&p, &plan), size_text);  // before reserved, before the options
    p.struct_size = sizeof(p);
    EXPECT(fn(&p, &plan), n + reserved_text);  // before the options
    p.reserved = 0;
    EXPECT(fn(&p, &plan), std::string("BMQCRC_F_PLAN does not apply to ") + call);
    EXPECT(fn(&p, &host),
           std::string(call) + " takes device pointers only: BMQCRC_F_DEVICE_PTRS is required");
    EXPECT(fn(&p, nullptr),
           std::string(call) + " takes device pointers only: BMQCRC_F_DEVICE_PTRS is required");
}

int main()
{
    preamble<bmqcrc_put_pack>("bmqcrc_put_pack", "bmqcrc_put_event_pack",
                              [](const bmqcrc_put_pack* p, const bmqcrc_opts* o) {
                                  return bmqcrc_put_event_pack(p, nullptr, o);
                              });
    preamble<bmqcrc_records_pack>("bmqcrc_records_pack", "bmqcrc_message_records_pack",
                                  [](const bmqcrc_records_pack* p, const bmqcrc_opts* o) {
                                      return bmqcrc_message_records_pack(p, nullptr, o);
                                  });
    preamble<bmqcrc_put_unpack>("bmqcrc_put_unpack", "bmqcrc_put_event_unpack",
                                [](const bmqcrc_put_unpack* p, const bmqcrc_opts* o) {
                                    return bmqcrc_put_event_unpack(p, nullptr, o);
                                });
    preamble<bmqcrc_records_unpack>("bmqcrc_records_unpack", "bmqcrc_message_records_unpack",
                                    [](const bmqcrc_records_unpack* p, const bmqcrc_opts* o) {
                                        return bmqcrc_message_records_unpack(p, nullptr, o);
                                    });
    preamble<bmqcrc_journal_select_args>(
        "bmqcrc_journal_select_args", "bmqcrc_journal_select",
        [](const bmqcrc_journal_select_args* p, const bmqcrc_opts* o) {
            return bmqcrc_journal_select(p, nullptr, o);
        },
        ".reserved and reserved2 must be 0");
    const bmqcrc_opts good = options(BMQCRC_F_DEVICE_PTRS);
    {
        bmqcrc_journal_select_args p;
        memset(&p, 0, sizeof(p));
        p.struct_size = sizeof(p);
        p.reserved2 = -1;
        EXPECT(bmqcrc_journal_select(&p, nullptr, &good),
               "bmqcrc_journal_select_args.reserved and reserved2 must be 0");
    }
    // The overlap tables: addresses inside one arena, nothing of it is read.
    alignas(8) static uint8_t arena[1 << 18];
    uint8_t* const in = arena + (1 << 16);   // an input of 4,096 bytes
    uint8_t* const in2 = arena + (1 << 17);  // another
    {
        bmqcrc_put_unpack p;
        memset(&p, 0, sizeof(p));
        p.struct_size = sizeof(p);
        p.events = in;
        p.events_bytes = 4096;
        p.n_events = 1;
        p.msg_cap = 64;
        p.app_offsets = (uint64_t*)arena;
        p.lengths = (uint32_t*)(arena + 1024);
        p.flags = in + 4095;         // its first byte is the input's last
        p.guids = in - 16 * 64 + 1;  // its last byte is the input's first
        EXPECT(bmqcrc_put_event_unpack(&p, nullptr, &good),
               "guids overlaps [events, events+events_bytes)");  // the table's order
        p.guids = in - 16 * 64;      // ends where the input begins
        EXPECT(bmqcrc_put_event_unpack(&p, nullptr, &good),
               "flags overlaps [events, events+events_bytes)");
        p.flags = nullptr;
        p.event_first = (uint64_t*)(in + 4088);  // n_events + 1 entries
        EXPECT(bmqcrc_put_event_unpack(&p, nullptr, &good),
               "event_first overlaps [events, events+events_bytes)");
    }
    {
        bmqcrc_records_unpack p;
        memset(&p, 0, sizeof(p));
        p.struct_size = sizeof(p);
        p.journal = in;
        p.journal_bytes = 60 * 68;
        p.n_records = 68;
        p.data = in2;
        p.data_bytes = 4096;
        p.msg_cap = 64;
        p.app_offsets = (uint64_t*)arena;
        p.lengths = (uint32_t*)(arena + 1024);
        p.record_index = (uint32_t*)in2;  // output-major: the first output, though it meets `data`
        p.expected = (uint32_t*)in;       // and a later one meets the journal
        EXPECT(bmqcrc_message_records_unpack(&p, nullptr, &good),
               "record_index overlaps [data, data+data_bytes)");
        p.record_index = p.expected = nullptr;
        p.out = (uint32_t*)(in + 60 * 68);  // one output meeting both: the journal is named
        p.journal_bytes = 60 * 68 + 24;
        p.data = in + 4096;
        p.data_bytes = 64;
        EXPECT(bmqcrc_message_records_unpack(&p, nullptr, &good),
               "out overlaps [journal, journal+journal_bytes)");
        p.journal_bytes = 60 * 68;
        EXPECT(bmqcrc_message_records_unpack(&p, nullptr, &good),
               "out overlaps [data, data+data_bytes)");
    }
    printf(g_fail ? "FAIL: %d\n" : "PASS\n", g_fail);
    return g_fail != 0;
}
