// packet_fec_host.cpp -- dab-radio_amd/csrc/packet_fec_core.h and dabgpu_packet_tx_layout on the host (tests/test_packet_fec_host.py).
//   packet_fec_host tables OUT            the row -> ring offset map [12][204] (u16) and its inverse over the FEC packets [9][24] (i16)
//   packet_fec_host walk IN OUT           buffers (u32 count, then u32 length + bytes each) through the walk and the ring arithmetic, without
//                                         the row decoder: per ReadPacket six i32 = consumed, stored, is_fec, ring fill, read head, event
//                                         (0 none, 1 everything handed out uncorrected, 2 frame corrected); then per buffer... the CRC of it
//   packet_fec_host fuzz SEED ROUNDS      hostile inputs to the layout and the walk, invariants checked here; built with
//                                         -fsanitize=address,undefined by the test and run directly
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "dabgpu.h"
#include "packet_fec_core.h"

using namespace dabgpu::pkt;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); abort(); } } while (0)

struct HostRing {
    std::vector<uint8_t> ring = std::vector<uint8_t>(RING_BYTES);      // exactly the ring: the sanitizer sees any index beyond it
    int read = 0, write = 0, size = 0, last = -1, discarded = 0;
    // -> consumed; fills the trace record
    int read_packet(const uint8_t* buf, int remain, int32_t* rec) {
        Header h{};
        bool stored = false;
        const int used = walk_step(remain, buf[0], remain >= 2 ? buf[1] : (uint8_t)0, &h, &stored);
        int event = 0;
        if (stored) {
            while (ring_free(size) < h.length) {
                const int other = packet_length(ring[read] >> 6);
                size -= other; read = ring_at(read, other); discarded++;
            }
            for (int k = 0; k < h.length; k++) ring[ring_at(write, k)] = (k == 0) ? stored_header(buf[0], h.length_id) : buf[k];
            size += h.length; write = ring_at(write, h.length);
            if (h.is_fec) {
                if (fec_counter_invalid(last, h.counter)) { last = -1; event = 1; pop_all(); }
                else {
                    last = h.counter;
                    if (h.counter == FEC_PACKETS - 1) {
                        event = (size == RING_BYTES) ? 2 : 1;
                        pop_all();
                        last = -1; read = write = size = 0;
                    }
                }
            }
        }
        if (rec) { rec[0] = used; rec[1] = stored; rec[2] = stored ? h.is_fec : 0; rec[3] = size; rec[4] = read; rec[5] = event; }
        return used;
    }
    void pop_all() {
        while (size > 0) {
            const int n = packet_length(ring[read] >> 6);
            CHECK(size >= n);
            size -= n; read = ring_at(read, n);
        }
    }
};

static uint32_t rd32(FILE* f) { uint32_t v = 0; if (fread(&v, 4, 1, f) != 1) return 0; return v; }

static uint64_t rng_state = 1;
static uint32_t rnd() { rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(rng_state >> 33); }

static void fuzz_layout() {
    const uint32_t lengths[] = {24, 48, 72, 96, 0, 25, 120};
    const uint32_t address = (rnd() % 8 == 0) ? rnd() % 2048 : 1 + rnd() % 1021;
    const uint32_t L = lengths[rnd() % ((rnd() % 8 == 0) ? 7 : 4)];
    const uint32_t fb = (rnd() % 10 == 0) ? rnd() % 200 : 24 * (1 + rnd() % 80);
    const uint64_t start = (rnd() % 10 == 0) ? rnd() : 24ull * (rnd() % 100000);
    const int K = (int)(rnd() % 4);
    std::vector<uint32_t> groups(rnd() % 24);
    for (auto& g : groups) g = (rnd() % 16 == 0) ? rnd() % 10000 : rnd() % 600;
    std::vector<dabgpu_packet_tx_entry> table((size_t)MAX_FRAME_PACKETS * (size_t)K);   // exactly what the call may fill
    std::vector<uint32_t> first((size_t)K + 1);
    size_t consumed = 99;
    uint64_t end_start = 0;
    uint32_t end_ci = 0;
    const uint32_t ci = rnd() % 4;
    const int st = dabgpu_packet_tx_layout(groups.data(), groups.size(), address, L, fb, start, ci, K, table.data(), table.size(), first.data(),
                                           &consumed, &end_start, &end_ci);
    if (st != 0) { CHECK(consumed == 0); return; }
    CHECK(address >= 1 && address <= 1021 && length_valid((int)L) && fb % 24 == 0 && fb >= L && start % 24 == 0);
    CHECK(consumed <= groups.size() && end_start == start + (uint64_t)K * RING_BYTES && first[0] == 0);
    uint32_t n_data = 0;
    for (int t = 0; t < K; t++) {
        uint32_t pos = (uint32_t)t * RING_BYTES;
        CHECK(first[t + 1] > first[t] && first[t + 1] - first[t] <= (uint32_t)MAX_FRAME_PACKETS);
        for (uint32_t i = first[t]; i < first[t + 1]; i++) {
            const dabgpu_packet_tx_entry& e = table[i];
            CHECK(e.position == pos && length_valid(e.length) && e.useful + 5 <= e.length);
            CHECK((start + pos) % fb + e.length <= fb);
            CHECK(e.group >= -1 && e.group < (int32_t)consumed);
            if (e.group >= 0) { CHECK(e.length == L && e.offset + e.useful <= groups[e.group] && e.continuity_index == ((ci + n_data) & 3)); n_data++; }
            else CHECK(e.length == 24 && e.useful == 0);
            pos += e.length;
        }
        CHECK(pos == (uint32_t)t * RING_BYTES + APP_TABLE_BYTES);
    }
    CHECK(end_ci == ((ci + n_data) & 3));
}

static void fuzz_walk() {
    HostRing r;
    const int n_bufs = 1 + rnd() % 6;
    for (int b = 0; b < n_bufs; b++) {
        const size_t n = rnd() % 4000;
        std::vector<uint8_t> buf(n);
        for (auto& v : buf) v = (uint8_t)rnd();
        // make FEC packets likely: sprinkle the address, sometimes with running counters
        for (size_t k = 0; k + 24 <= n; k += 24) if (rnd() % 3 == 0) { buf[k] = (uint8_t)(((rnd() % 4) << 6) | ((rnd() % 10) << 2) | 3); buf[k + 1] = 0xFE; }
        size_t at = 0;
        while (at < n) {
            std::vector<uint8_t> rest(buf.begin() + at, buf.end());                      // an exact copy: reads past the remainder are seen
            int32_t rec[6];
            const int used = r.read_packet(rest.data(), (int)rest.size(), rec);
            CHECK(used > 0 && (size_t)used <= rest.size());
            CHECK(r.size >= 0 && r.size <= RING_BYTES && r.read >= 0 && r.read < RING_BYTES && r.write >= 0 && r.write < RING_BYTES);
            CHECK(r.size % 24 == 0);
            at += (size_t)used;
        }
    }
    std::vector<uint8_t> p(24 * (1 + rnd() % 4));
    for (auto& v : p) v = (uint8_t)rnd();
    const uint16_t c = crc16(p.data(), (int)p.size() - 2);
    p[p.size() - 2] = (uint8_t)(c >> 8); p[p.size() - 1] = (uint8_t)c;
    CHECK(packet_crc_ok(p.data(), (int)p.size()));
    p[rnd() % p.size()] ^= (uint8_t)(1u << (rnd() % 8));
    CHECK(!packet_crc_ok(p.data(), (int)p.size()));
}

int main(int argc, char** argv) {
    if (argc >= 3 && !strcmp(argv[1], "tables")) {
        FILE* out = fopen(argv[2], "wb");
        if (!out) return 2;
        std::vector<int> seen(RING_BYTES, 0);
        for (int y = 0; y < RS_ROWS; y++)
            for (int x = 0; x < RS_MESSAGE_BYTES; x++) {
                const int o = row_symbol_offset(y, x);
                CHECK(o >= 0 && o < RING_BYTES && !seen[o]);
                seen[o] = 1;
                const uint16_t v = (uint16_t)o;
                fwrite(&v, 2, 1, out);
            }
        for (int m = 0; m < FEC_PACKETS; m++)
            for (int k = 0; k < FEC_PACKET_BYTES; k++) {
                const int16_t t = (int16_t)fec_packet_table_index(m, k);
                if (t >= 0) CHECK(row_symbol_offset(t % RS_ROWS, RS_DATA_BYTES + t / RS_ROWS) == APP_TABLE_BYTES + m * FEC_PACKET_BYTES + k);
                fwrite(&t, 2, 1, out);
            }
        fclose(out);
        return 0;
    }
    if (argc >= 4 && !strcmp(argv[1], "walk")) {
        FILE* in = fopen(argv[2], "rb");
        FILE* out = fopen(argv[3], "wb");
        if (!in || !out) return 2;
        HostRing r;
        const uint32_t n_bufs = rd32(in);
        for (uint32_t b = 0; b < n_bufs; b++) {
            const uint32_t n = rd32(in);
            std::vector<uint8_t> buf(n);
            if (n && fread(buf.data(), 1, n, in) != n) return 3;
            size_t at = 0;
            while (at < n) {
                int32_t rec[6];
                at += (size_t)r.read_packet(buf.data() + at, (int)(n - at), rec);
                fwrite(rec, 4, 6, out);
            }
            const int32_t tail[6] = {-1, (int32_t)crc16(buf.data(), (int)n), r.discarded, 0, 0, 0};
            fwrite(tail, 4, 6, out);
        }
        fclose(out);
        return 0;
    }
    if (argc >= 4 && !strcmp(argv[1], "fuzz")) {
        rng_state = strtoull(argv[2], nullptr, 10) * 2 + 1;
        const long rounds = strtol(argv[3], nullptr, 10);
        for (long i = 0; i < rounds; i++) { fuzz_layout(); fuzz_walk(); }
        printf("fuzz ok: %ld rounds\n", rounds);
        return 0;
    }
    fprintf(stderr, "usage: packet_fec_host tables OUT | walk IN OUT | fuzz SEED ROUNDS\n");
    return 2;
}
