// packet_fec_harness.cpp -- the packet-mode mirror classes on the device (tests/test_gpu_packet_class.py).
//   packet_fec_harness rx IN OUT   IN: u32 n_bufs, then u32 length + bytes each.  The buffers go through a fresh
//                                  MSC_Reed_Solomon_Data_Packet_Processor the way Basic_Data_Packet_Channel::ProcessFECPackets walks them
//                                  (src/basic_radio/basic_data_packet_channel.cpp:74-80).  OUT: u32 n_ret, the ReadPacket return values (u32),
//                                  u32 n_callbacks, u32 log bytes, the log: per callback flag (u8), length (u32), the packet
//   packet_fec_harness tx IN OUT   IN: u32 address, packet length, frame bytes, n_blocks; per block u32 n_fec_frames, n_groups, then u32 length +
//                                  bytes per group.  Groups a block did not take are offered to the next one before its own.
//                                  OUT: u32 n_frame_bytes, the logical frames (flushed at the end), u32 groups consumed in all
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "dab/msc/msc_reed_solomon_data_packet_processor.h"
#include "dab/tx/dab_packet_encoder.h"

static uint32_t rd32(FILE* f) { uint32_t v = 0; if (fread(&v, 4, 1, f) != 1) return 0; return v; }
static void wr32(FILE* f, uint32_t v) { fwrite(&v, 4, 1, f); }

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: packet_fec_harness rx|tx IN OUT\n"); return 2; }
    FILE* in = fopen(argv[2], "rb");
    FILE* out = fopen(argv[3], "wb");
    if (!in || !out) return 2;
    if (!strcmp(argv[1], "rx")) {
        MSC_Reed_Solomon_Data_Packet_Processor proc;
        std::vector<uint8_t> log;
        uint32_t n_cb = 0;
        proc.SetCallback([&](tcb::span<const uint8_t> p, bool corrected) {
            log.push_back(corrected ? 1 : 0);
            const uint32_t n = (uint32_t)p.size();
            for (int k = 0; k < 4; k++) log.push_back((uint8_t)(n >> (8 * k)));
            log.insert(log.end(), p.begin(), p.end());
            n_cb++;
        });
        std::vector<uint32_t> rets;
        const uint32_t n_bufs = rd32(in);
        for (uint32_t b = 0; b < n_bufs; b++) {
            const uint32_t len = rd32(in);
            std::vector<uint8_t> buf(len);
            if (len && fread(buf.data(), 1, len, in) != len) return 3;
            tcb::span<const uint8_t> rest(buf);
            while (!rest.empty()) {
                const size_t used = proc.ReadPacket(rest);
                rets.push_back((uint32_t)used);
                rest = rest.subspan(used);
            }
        }
        wr32(out, (uint32_t)rets.size());
        for (uint32_t r : rets) wr32(out, r);
        wr32(out, n_cb);
        wr32(out, (uint32_t)log.size());
        fwrite(log.data(), 1, log.size(), out);
    } else {
        const uint32_t address = rd32(in), length = rd32(in), fb = rd32(in), n_blocks = rd32(in);
        DAB_Packet_Encoder enc(address, length, fb);
        std::vector<std::vector<uint8_t>> pending;
        std::vector<uint8_t> frames;
        uint32_t total = 0;
        for (uint32_t b = 0; b < n_blocks; b++) {
            const uint32_t K = rd32(in), n_groups = rd32(in);
            for (uint32_t g = 0; g < n_groups; g++) {
                const uint32_t len = rd32(in);
                std::vector<uint8_t> grp(len);
                if (len && fread(grp.data(), 1, len, in) != len) return 3;
                pending.push_back(std::move(grp));
            }
            std::vector<tcb::span<const uint8_t>> spans(pending.begin(), pending.end());
            size_t consumed = 0;
            if (!enc.EncodeBlock(spans, (int)K, &consumed, frames)) { fprintf(stderr, "EncodeBlock refused: %d\n", enc.GetLastStatus()); return 4; }
            pending.erase(pending.begin(), pending.begin() + (ptrdiff_t)consumed);
            total += (uint32_t)consumed;
        }
        enc.Flush(frames);
        wr32(out, (uint32_t)frames.size());
        fwrite(frames.data(), 1, frames.size(), out);
        wr32(out, total);
    }
    fclose(out);
    return 0;
}
