// ref_packet_shim.cpp — C-ABI wrapper around the REFERENCE's own Packet (both variants) and
// opt Window, compiled from where they lie: oracle/Makefile passes -I$(REF)/cpp/src/<variant>
// and the reference's .cpp files on the same command line; nothing is copied.  Output goes to
// oracle/_ref/ only: libref_packet_base.so (base/Packet.cpp) and libref_packet_opt.so
// (opt/Packet.cpp, opt/Window.cpp, with -DREF_PACKET_WINDOW).  Two libraries, because both
// variants define `class Packet`; they are linked -Bsymbolic, so each binds its own.
//
// TEST INFRASTRUCTURE ONLY: used by tests/golden/make_wire_golden.py to record
// tests/golden/wire.json and by tests/test_wire_reference.py to replay it.  The product
// library never links or loads it.
//
// In reach: the serialisation (Packet(type, data, seq) + getNetworkOrderHeader(), what
// sendPacket puts on the wire), the parse (Packet(buf, size)) and the selective sender
// window (Window::markPacketAsAcked / determineWindowAdvance).
// Not in reach: base/Sender.cpp needs cxxopts, which the reference tree does not carry, and
// both receivers are socket loops inside main(), whose quirks are not
// to be mirrored.  So cumulative ingest and the receive window stay restatements
// (tests/retx_model.py, tests/accept_model.py, tests/ack_model.py).
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "Packet.hpp"  // reference: cpp/src/<variant>/Packet.hpp
#ifdef REF_PACKET_WINDOW
#include "Window.hpp"  // reference: cpp/src/opt/Window.hpp
#endif

extern "C" {

// Packet(type, data, seq) as sendPacket serialises it (base/Sender.cpp:187-197):
// getNetworkOrderHeader() then the data.  out holds 16 + len bytes.
void ref_packet_build(uint32_t type, const void *data, uint32_t len, uint32_t seq, uint8_t *out) {
    const char *d = static_cast<const char *>(data);
    const std::vector<char> v(d, d + len);
    const Packet p(type, v, seq);
    const PacketHeader h = p.getNetworkOrderHeader();
    static_assert(sizeof h == 16, "PacketHeader is 16 bytes");
    std::memcpy(out, &h, sizeof h);
    if (len) std::memcpy(out + sizeof h, p.getData().data(), len);
}

// Packet(buf, size) -> out = {type, seqNum, length, checksum, calculateCheckSum()}.
// The reference's constructor copies header.length bytes whatever `size` is (Packet.cpp:29-32),
// so the datagram is first copied into a zero-padded buffer that holds them; a length field
// above 65536 is refused (-1) rather than handed to it.  Also -1 for size < 16 (it throws).
int ref_packet_parse(const void *buf, size_t size, uint32_t *out) {
    if (size < 16) return -1;
    const uint8_t *b = static_cast<const uint8_t *>(buf);
    const uint32_t field = (uint32_t(b[8]) << 24) | (uint32_t(b[9]) << 16) | (uint32_t(b[10]) << 8) | uint32_t(b[11]);
    if (field > 65536) return -1;
    std::vector<char> padded(16 + (field > size - 16 ? field : size - 16), 0);
    std::memcpy(padded.data(), buf, size);
    const Packet p(padded.data(), size);
    out[0] = p.getType();
    out[1] = p.getSeqNum();
    out[2] = p.getLength();
    out[3] = p.getCheckSum();
    out[4] = p.calculateCheckSum();
    return 0;
}

#ifdef REF_PACKET_WINDOW
// Window(w); addPacket(Packet(DATAOPT, {}, seq0 + s)) for s < inflight; markPacketAsAcked for
// each ACK seqNum in order (opt/Sender.cpp:130-139); flags[s] = packetIsAcked() of every
// packet; returns determineWindowAdvance().  markPacketAsAcked prints a line per call: the
// caller silences file descriptors 1 and 2 around this function.
size_t ref_window_run(int w, uint32_t seq0, uint32_t inflight, const uint32_t *acks, size_t nacks, uint8_t *flags) {
    Window win(w);
    for (uint32_t s = 0; s < inflight; ++s) win.addPacket(Packet(DATAOPT, {}, seq0 + s));
    for (size_t i = 0; i < nacks; ++i) win.markPacketAsAcked(acks[i]);
    uint32_t s = 0;
    for (const Packet &p : win.getPackets()) flags[s++] = p.packetIsAcked() ? 1 : 0;
    return win.determineWindowAdvance();
}
#endif

}  // extern "C"
