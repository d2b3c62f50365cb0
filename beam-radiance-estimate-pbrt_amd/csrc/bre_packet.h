// bre_packet.h — the per-packet record of the tile gather and its sizing.  Plain C++ (no HIP): the host code
// that sizes and indexes the records is also compiled on its own by tests/packet_rec_check.cpp.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace bre {

// One 64-segment packet of a launch as the specialised tile kernel reads it (k_packet_prep writes it once
// per launch, next to k_seg_prep): the packet bundle of make_bundle (bre_gather.hip, `Bundle`, field for
// field) and the packet's largest lane margin Al'.  Every (packet, work root) wave reads its packet's record
// with scalar loads instead of forming the bundle again.  80 B, a multiple of 16.
struct alignas(16) PacketRec {
    float co[3], cu[3];
    float delta, omax;
    float s0, s1, gbox;
    float icu[3];
    float q[3];
    float col1;
    float al_max;  // max over the valid lanes of ScanLane::al below FLT_MAX (0 if none)
    float pad;     // 0
};
static_assert(sizeof(PacketRec) == 80 && sizeof(PacketRec) % 16 == 0, "PacketRec must be a multiple of 16 B");
constexpr int kPacketRecWords = (int)(sizeof(PacketRec) / sizeof(float));

// Packets (and records) of a launch of nseg segments: the last one may hold fewer than 64 valid lanes.
constexpr int64_t packet_count(int64_t nseg) { return nseg <= 0 ? 0 : (nseg + 63) / 64; }
// The record of the packet whose first segment is seg0 (a multiple of 64), counted within the LAUNCH: a
// packet shard's and a later launch's segments are renumbered from 0, and so are their records.
constexpr int64_t packet_index(int64_t seg0) { return seg0 >> 6; }

// Segments per launch of a gather of nseg segments that keeps per_seg bytes of partial sums per segment
// within partial_cap: whole packets, at most 2^26 (the exact stage's 32-bit record offsets), at least one
// packet, never more than the gather (gather_device, bre_api_gather.hip).
inline int64_t launch_chunk(int64_t nseg, int64_t partial_cap, size_t per_seg) {
    int64_t chunk = partial_cap / (int64_t)per_seg / 64 * 64;
    if (chunk > ((int64_t)1 << 26)) chunk = (int64_t)1 << 26;
    if (chunk < 64) chunk = 64;
    if (chunk > nseg) chunk = nseg;
    return chunk;
}

}  // namespace bre
