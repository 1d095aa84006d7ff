// packet_fec_core.h -- the arithmetic of MSC packet mode and its FEC scheme (EN 300 401 clauses 5.3.2 and 5.3.5) that the kernels
// (packet_fec.hip), the transmit planner (dabgpu_host_logic.cpp) and the host tests share: packet lengths, the header parse and the walk
// step of MSC_Reed_Solomon_Data_Packet_Processor::ReadPacket (src/dab/msc/msc_reed_solomon_data_packet_processor.cpp:57-87), the ring
// arithmetic (:132-184), the row <-> ring index maps of the RS(204,188) rows (:186-222) and the packet CRC
// (src/dab/msc/msc_data_packet_processor.cpp:23-32,81-92).  Plain C++, no HIP headers, no tables in memory.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PKT_HD __host__ __device__
#else
#define PKT_HD
#endif

namespace dabgpu {
namespace pkt {

constexpr int RS_DATA_BYTES = 188, RS_PARITY_BYTES = 16, RS_MESSAGE_BYTES = 204, RS_ROWS = 12, RS_PADDING = 51;
constexpr int APP_TABLE_BYTES = 2256;                    // 188 x 12 application bytes of a FEC frame
constexpr int RS_TABLE_BYTES = 192;                      // 16 x 12 parity bytes
constexpr int FEC_PACKET_BYTES = 24, FEC_PACKETS = 9, FEC_DATA_FIELD = 22, FEC_PAD_BYTES = 6;
constexpr int RING_BYTES = APP_TABLE_BYTES + FEC_PACKETS * FEC_PACKET_BYTES;        // 2472
constexpr int FEC_ADDRESS = 0x3FE;
constexpr int MAX_RING_PACKETS = RING_BYTES / 24;        // 103
constexpr int MAX_FRAME_PACKETS = APP_TABLE_BYTES / 24;  // 94
constexpr int MAX_GROUP_BYTES = 8191;
constexpr int MAX_ADDRESS = 1021;

PKT_HD inline int packet_length(int length_id) { return 24 * ((length_id & 3) + 1); }           // table 6: 24 / 48 / 72 / 96
PKT_HD inline int length_id_of(int length) { return length / 24 - 1; }
PKT_HD inline bool length_valid(int length) { return length == 24 || length == 48 || length == 72 || length == 96; }

// the two header bytes as the FEC layer reads them (:64-75): a FEC packet's length field is not believed
struct Header {
    int length_id, counter, address, is_fec, length;
};
PKT_HD inline Header parse_header(uint8_t b0, uint8_t b1) {
    Header h;
    h.length_id = (b0 >> 6) & 3;
    h.counter = (b0 >> 2) & 15;
    h.address = ((b0 & 3) << 8) | b1;
    h.is_fec = (h.address == FEC_ADDRESS);
    if (h.is_fec) h.length_id = 0;
    h.length = packet_length(h.length_id);
    return h;
}
// the header byte as the ring stores it (:150-152)
PKT_HD inline uint8_t stored_header(uint8_t b0, int length_id) { return (uint8_t)((b0 & 0x3F) | ((length_id & 3) << 6)); }

// one ReadPacket over `remain` bytes: the bytes consumed; *stored = whether a packet (described by *h) goes into the ring.  A remainder
// shorter than two bytes or than the packet its header names is consumed without being stored (:58-61, :78-81); b0, b1 are only looked
// at when remain >= 2.
PKT_HD inline int walk_step(int remain, uint8_t b0, uint8_t b1, Header* h, bool* stored) {
    *stored = false;
    if (remain < 2) return remain;
    *h = parse_header(b0, b1);
    if (remain < h->length) return remain;
    *stored = true;
    return h->length;
}

// whether a FEC packet's counter breaks the 0..8 sequence (:89-98); last < 0 = no counter remembered
PKT_HD inline bool fec_counter_invalid(int last, int counter) { return (last >= 0) ? (((last + 1) & 0xFF) != counter) : (counter != 0); }

// ring arithmetic (:136-147, :157-158, :173-174)
PKT_HD inline int ring_at(int head, int offset) { int k = head + offset; return (k >= RING_BYTES) ? k - RING_BYTES : k; }   // head, offset < RING
PKT_HD inline int ring_free(int size) { return RING_BYTES - size; }

// symbol x (0..203) of row y (0..11) as a byte offset behind the ring's read head (:190-222): application byte x*12 + y, or byte
// t = (x - 188)*12 + y of the RS data table = data field byte t % 22 of FEC packet t / 22
PKT_HD inline int row_symbol_offset(int y, int x) {
    if (x < RS_DATA_BYTES) return x * RS_ROWS + y;
    const int t = (x - RS_DATA_BYTES) * RS_ROWS + y;
    return APP_TABLE_BYTES + (t / FEC_DATA_FIELD) * FEC_PACKET_BYTES + 2 + t % FEC_DATA_FIELD;
}
// the inverse for the transmitter: byte k (0..23) of FEC packet m (0..8) -> RS table index, or -1 for header and padding bytes
PKT_HD inline int fec_packet_table_index(int m, int k) {
    if (k < 2) return -1;
    const int t = m * FEC_DATA_FIELD + (k - 2);
    return (t < RS_TABLE_BYTES) ? t : -1;
}
PKT_HD inline uint8_t fec_packet_header0(int m) { return (uint8_t)(((m & 15) << 2) | (FEC_ADDRESS >> 8)); }
PKT_HD inline uint8_t fec_packet_header1() { return (uint8_t)(FEC_ADDRESS & 0xFF); }

// CRC-16 x^16+x^12+x^5+1, start 0xFFFF, inverted (msc_data_packet_processor.cpp:23-32), bit by bit
PKT_HD inline uint16_t crc16(const uint8_t* p, int n) {
    uint32_t c = 0xFFFFu;
    for (int i = 0; i < n; i++) {
        c ^= (uint32_t)p[i] << 8;
        for (int b = 0; b < 8; b++) c = (c & 0x8000u) ? (((c << 1) ^ 0x1021u) & 0xFFFFu) : ((c << 1) & 0xFFFFu);
    }
    return (uint16_t)(c ^ 0xFFFFu);
}
// a data packet's check (:81-92): over the first length - 2 bytes, compared big-endian with the last two
PKT_HD inline bool packet_crc_ok(const uint8_t* p, int length) {
    const uint16_t c = crc16(p, length - 2);
    return p[length - 2] == (uint8_t)(c >> 8) && p[length - 1] == (uint8_t)(c & 0xFF);
}

// the data-packet header (figure 11; msc_data_packet_processor.cpp:60-66)
PKT_HD inline uint8_t data_header0(int length_id, int ci, int first, int last, int address) {
    return (uint8_t)(((length_id & 3) << 6) | ((ci & 3) << 4) | ((first & 1) << 3) | ((last & 1) << 2) | ((address >> 8) & 3));
}

// where byte `rel` of a call that begins at stream byte start_byte lands: logical frame (relative to the one holding start_byte) and column
PKT_HD inline void frame_position(uint64_t start_byte, uint64_t rel, uint32_t frame_bytes, uint64_t* frame, uint32_t* column) {
    const uint64_t k = start_byte + rel;
    *frame = k / frame_bytes - start_byte / frame_bytes;
    *column = (uint32_t)(k % frame_bytes);
}

}  // namespace pkt
}  // namespace dabgpu
