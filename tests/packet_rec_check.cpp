// csrc/bre_packet.h on the host: the sizing of a launch's packet records and their indexing, walked the way
// gather_device (bre_api_gather.hip) and the specialised tile kernel use them.  Built with the host compiler
// under AddressSanitizer and UBSan by tests/test_packet_rec_host.py; prints "<n> failures".
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "bre_packet.h"

using namespace bre;

static int failures = 0;
#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            ++failures;                                           \
            printf("line %d: %s\n", __LINE__, #c);                \
        }                                                         \
    } while (0)

// One gather of nseg segments as gather_device runs it: a buffer of packet_count(chunk) records, then launches
// of at most `chunk` segments, each writing one record per packet (the writer's grid) and each of its tile
// waves reading record packet_index(seg0).  Every read must hit a record the same launch wrote.
static void walk(int64_t nseg, int64_t partial_cap, size_t per_seg) {
    const int64_t chunk = launch_chunk(nseg, partial_cap, per_seg);
    CHECK(chunk >= 1 && chunk <= nseg);
    CHECK(chunk == nseg || chunk % 64 == 0);  // every launch but the last starts and ends on a packet
    CHECK(chunk <= ((int64_t)1 << 26));
    std::vector<PacketRec> buf((size_t)packet_count(chunk));
    std::vector<int> stamp(buf.size(), -1);
    int launch = 0;
    int64_t covered = 0;
    for (int64_t off = 0; off < nseg; off += chunk, ++launch) {
        const int64_t n = chunk < nseg - off ? chunk : nseg - off;
        const int64_t npk = packet_count(n);
        CHECK(npk >= 1 && (size_t)npk <= buf.size());
        for (int64_t b = 0; b < npk; ++b) {  // the writer: workgroup b stores record b
            buf[(size_t)b].al_max = (float)(off + 64 * b);
            stamp[(size_t)b] = launch;
        }
        for (int64_t grp = 0; grp < npk; ++grp) {  // the tile kernel: packet group grp, lane 0 is seg0
            const int64_t seg0 = grp * 64;
            CHECK(seg0 < n);
            const int64_t r = packet_index(seg0);
            CHECK(r >= 0 && r < npk);
            CHECK(stamp[(size_t)r] == launch);
            CHECK(buf[(size_t)r].al_max == (float)(off + seg0));  // this launch's packet, not the film's
        }
        covered += n;
    }
    CHECK(covered == nseg);
}

int main() {
    static_assert(sizeof(PacketRec) % 16 == 0, "a multiple of 16 B");
    static_assert(kPacketRecWords == 20, "nineteen values and a pad");
    CHECK(packet_count(0) == 0 && packet_count(-5) == 0);
    CHECK(packet_count(1) == 1 && packet_count(64) == 1 && packet_count(65) == 2 && packet_count(129) == 3);
    CHECK(packet_count((int64_t)1 << 26) == ((int64_t)1 << 20));
    CHECK(packet_index(0) == 0 && packet_index(64) == 1 && packet_index(((int64_t)1 << 26) - 64) == ((int64_t)1 << 20) - 1);
    const int64_t gib4 = (int64_t)4 << 30, mib1 = (int64_t)1 << 20;
    // the default cap: C2's ~0.6 M segments at S = 256 in one launch
    CHECK(launch_chunk(603441, gib4, 256 * 12) == 603441);
    // option 109 at 1 MiB: 320 segments per launch at S = 256, 192 with counts; never below one packet
    CHECK(launch_chunk(400, mib1, 256 * 12) == 320);
    CHECK(launch_chunk(400, mib1, 256 * 20) == 192);
    CHECK(launch_chunk(400, mib1, (size_t)1 << 20) == 64);
    CHECK(launch_chunk(10, mib1, (size_t)1 << 20) == 10);
    // a tiny per-segment cost cannot pass the exact stage's 2^26 segments per launch
    CHECK(launch_chunk((int64_t)1 << 28, (int64_t)1 << 40, 12) == ((int64_t)1 << 26));
    for (int64_t nseg : {1, 63, 64, 65, 129, 200, 320, 321, 400, 640, 641, 4000})
        for (size_t per_seg : {(size_t)12, (size_t)256 * 12, (size_t)256 * 20, (size_t)1 << 20}) {
            walk(nseg, mib1, per_seg);
            walk(nseg, gib4, per_seg);
        }
    // a packet shard's m segments (bre_shard_segments) are gathered as a launch of their own: records 0 .. m/64
    for (int64_t m : {64, 72, 128, 136}) walk(m, gib4, 256 * 12);
    printf("%d failures\n", failures);
    return failures != 0;
}
