// The reference's three Fiat-Shamir transcripts (src/transcript/{merlin,keccak256,blake3}.rs), the verifier's challenges
// (src/verifier.rs:24-42 with src/common.rs:21-98) and the prover's (src/prover.rs:125-138, 189) as PM_HD code: fixed-size, streaming restatements of host/hashes.hpp and of the
// transcript classes and Polymath::verifier_challenges of host/polymath.hpp -- those two files are the specification, bit for bit
// (tests/native/transcript_selftest.cpp compares every piece on the CPU).  No allocation: each state is a POD that one lane owns,
// and no message is ever laid out as one buffer -- the pieces (label bytes, a u64 length prefix, an Fr as its 32 canonical bytes,
// a compressed point record) are absorbed as they are produced, up to 8 bytes per step.
//
//   state                  bytes   what it keeps
//   Keccak256Stream          208   25 lanes, the position in the 136-byte rate
//   Blake3Stream             888   the chunk's chaining value, one 64-byte block, a stack of 24 chaining values
//   Strobe128 / Merlin       208   25 lanes, pos, pos_begin
//
// Absorption is word-wise: a piece of up to 8 bytes is shifted to its byte position and XORed into one or two lanes.  The lane
// index is a run-time value, so on the device a state lives in private memory between permutations; keccak_f1600 and b3_compress
// are real calls (PM_HD_COLD) that load it, run fully unrolled on registers and store it again: 400 bytes of traffic against
// ~7 000 instructions of permutation.
#pragma once
#include <stddef.h>
#include <string.h>

#include "field.cuh"

namespace pm {
namespace fs {

enum { KIND_MERLIN = 0, KIND_KECCAK256 = 1, KIND_BLAKE3 = 2 };   // pm_transcript (include/polymath_hip.h)

// ---------------------------------------------------------------------------------------------------------- Keccak-f[1600]
struct KeccakTables {
    static constexpr uint64_t RC[24] = {
        0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808Aull, 0x8000000080008000ull, 0x000000000000808Bull,
        0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008Aull, 0x0000000000000088ull,
        0x0000000080008009ull, 0x000000008000000Aull, 0x000000008000808Bull, 0x800000000000008Bull, 0x8000000000008089ull,
        0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800Aull, 0x800000008000000Aull,
        0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
    static constexpr unsigned RHO[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};
};

PM_HD uint64_t rol64(uint64_t v, unsigned n) { return n ? (v << n) | (v >> (64 - n)) : v; }

// hashes.hpp: keccak_f1600, every loop unrolled: lane indices, rotation counts and round constants are compile-time constants.
// (A template, as b3_compress below, so that every translation unit that includes this header may define it.)
template <int = 0>
PM_HD_COLD void keccak_f1600(uint64_t st[25]) {
    uint64_t a[25];
#pragma unroll
    for (int i = 0; i < 25; ++i) a[i] = st[i];
#pragma unroll
    for (int rnd = 0; rnd < 24; ++rnd) {
        uint64_t c[5], d[5], b[25];
#pragma unroll
        for (int x = 0; x < 5; ++x) c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
#pragma unroll
        for (int x = 0; x < 5; ++x) d[x] = c[(x + 4) % 5] ^ rol64(c[(x + 1) % 5], 1);
#pragma unroll
        for (int i = 0; i < 25; ++i) b[i / 5 + 5 * ((2 * (i % 5) + 3 * (i / 5)) % 5)] = rol64(a[i] ^ d[i % 5], KeccakTables::RHO[i]);
#pragma unroll
        for (int y = 0; y < 25; y += 5)
#pragma unroll
            for (int x = 0; x < 5; ++x) a[y + x] = b[y + x] ^ (~b[y + (x + 1) % 5] & b[y + (x + 2) % 5]);
        a[0] ^= KeccakTables::RC[rnd];
    }
#pragma unroll
    for (int i = 0; i < 25; ++i) st[i] = a[i];
}

PM_HD uint64_t low_bytes(uint64_t v, uint32_t n) { return n >= 8 ? v : v & (((uint64_t)1 << (8 * n)) - 1); }
PM_HD uint64_t load_le(const uint8_t *p, uint32_t n) {   // n <= 8 bytes, any alignment
    uint64_t v = 0;
    if (n == 8) memcpy(&v, p, 8);
    else for (uint32_t i = 0; i < n; ++i) v |= (uint64_t)p[i] << (8 * i);
    return v;
}
// words[] as a little-endian byte string: XOR the n <= 8 bytes of v in at byte `at` (v has no bits above 8 n)
PM_HD void xor_bytes_at(uint64_t *words, uint32_t at, uint64_t v, uint32_t n) {
    const uint32_t w = at >> 3, s = (at & 7) * 8;
    words[w] ^= v << s;
    if (s + 8 * n > 64) words[w + 1] ^= v >> (64 - s);
}

// Every stream below has absorb_le(v, n): the n <= 8 low bytes of v, least significant first.  absorb_bytes feeds a byte string
// through it.
template <class S>
PM_HD void absorb_bytes(S &s, const uint8_t *p, size_t n) {
    size_t i = 0;
    for (; i + 8 <= n; i += 8) s.absorb_le(load_le(p + i, 8), 8);
    if (i < n) s.absorb_le(load_le(p + i, (uint32_t)(n - i)), (uint32_t)(n - i));
}

// --------------------------------------------------------------------------------------------------------------- Keccak-256
// hashes.hpp: keccak256 = keccak_sponge256(data, 0x01): legacy padding 0x01 .. 0x80, rate 136
struct Keccak256Stream {
    static constexpr uint32_t RATE = 136;
    uint64_t st[25];
    uint32_t pos;
    PM_HD void init() {
        for (int i = 0; i < 25; ++i) st[i] = 0;
        pos = 0;
    }
    PM_HD void absorb_le(uint64_t v, uint32_t n) {
        while (n) {
            const uint32_t take = n < RATE - pos ? n : RATE - pos;
            xor_bytes_at(st, pos, low_bytes(v, take), take);
            pos += take;
            if (pos == RATE) { keccak_f1600(st); pos = 0; }
            v = take >= 8 ? 0 : v >> (8 * take);
            n -= take;
        }
    }
    PM_HD void absorb(const uint8_t *p, size_t n) { absorb_bytes(*this, p, n); }
    // the digest as 4 little-endian words; the state is spent
    PM_HD void finish(uint64_t d[4]) {
        xor_bytes_at(st, pos, 0x01, 1);
        xor_bytes_at(st, RATE - 1, 0x80, 1);
        keccak_f1600(st);
        for (int i = 0; i < 4; ++i) d[i] = st[i];
    }
    PM_HD void finish(uint8_t out32[32]) {
        uint64_t d[4];
        finish(d);
        memcpy(out32, d, 32);
    }
};

// ------------------------------------------------------------------------------------------------------------------- BLAKE3
struct B3Tables {
    static constexpr uint32_t IV[8] = {0x6A09E667, 0xBB67AE85, 0x3C6EF372, 0xA54FF53A, 0x510E527F, 0x9B05688C, 0x1F83D9AB, 0x5BE0CD19};
    static constexpr int PERM[16] = {2, 6, 3, 10, 7, 0, 4, 13, 1, 11, 12, 5, 9, 14, 15, 8};
};
enum { B3_CHUNK_START = 1, B3_CHUNK_END = 2, B3_PARENT = 4, B3_ROOT = 8 };

PM_HD uint32_t ror32(uint32_t v, int n) { return (v >> n) | (v << (32 - n)); }
#define PM_B3_G(a, b, c, d, mx, my)                                                                      \
    do {                                                                                                 \
        s[a] = s[a] + s[b] + (mx); s[d] = ror32(s[d] ^ s[a], 16); s[c] = s[c] + s[d]; s[b] = ror32(s[b] ^ s[c], 12); \
        s[a] = s[a] + s[b] + (my); s[d] = ror32(s[d] ^ s[a], 8);  s[c] = s[c] + s[d]; s[b] = ror32(s[b] ^ s[c], 7);  \
    } while (0)

// hashes.hpp: b3::compress; the block as 8 little-endian 64-bit words.  out may be cv.
template <int = 0>
PM_HD_COLD void b3_compress(const uint32_t cv[8], const uint64_t block[8], uint64_t counter, uint32_t blen, uint32_t flags, uint32_t out[8]) {
    uint32_t s[16], m[16], t[16];
#pragma unroll
    for (int i = 0; i < 8; ++i) { s[i] = cv[i]; m[2 * i] = (uint32_t)block[i]; m[2 * i + 1] = (uint32_t)(block[i] >> 32); }
#pragma unroll
    for (int i = 0; i < 4; ++i) s[8 + i] = B3Tables::IV[i];
    s[12] = (uint32_t)counter; s[13] = (uint32_t)(counter >> 32); s[14] = blen; s[15] = flags;
#pragma unroll
    for (int r = 0; r < 7; ++r) {
        PM_B3_G(0, 4, 8, 12, m[0], m[1]); PM_B3_G(1, 5, 9, 13, m[2], m[3]); PM_B3_G(2, 6, 10, 14, m[4], m[5]); PM_B3_G(3, 7, 11, 15, m[6], m[7]);
        PM_B3_G(0, 5, 10, 15, m[8], m[9]); PM_B3_G(1, 6, 11, 12, m[10], m[11]); PM_B3_G(2, 7, 8, 13, m[12], m[13]); PM_B3_G(3, 4, 9, 14, m[14], m[15]);
#pragma unroll
        for (int i = 0; i < 16; ++i) t[i] = m[B3Tables::PERM[i]];
#pragma unroll
        for (int i = 0; i < 16; ++i) m[i] = t[i];
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) out[i] = s[i] ^ s[i + 8];
}
#undef PM_B3_G

// hashes.hpp: blake3 (plain hash, 32 bytes out) as a stream: 64-byte blocks, 1024-byte chunks, and the chunk tree of
// b3::merge -- the left subtree of k chunks takes the largest power of two below k -- built bottom-up on a stack: when chunk
// number t (counted from 1) is complete and more input follows, its chaining value is merged with the stack's top once per
// trailing zero bit of t and pushed.  The stack then holds one entry per set bit of t: 24 entries serve t < 2^24, i.e.
// messages of up to 2^24 chunks = 2^34 bytes (16 GiB); a longer message would overrun it and is the caller's to refuse.
// A block and a chunk are closed only when more input arrives: the last block carries CHUNK_END, and ROOT if it is the only chunk.
struct Blake3Stream {
    static constexpr int STACK = 24;
    uint32_t cv[8];      // chaining value of the chunk in progress
    uint64_t buf[8];     // the block in progress
    uint64_t chunk;      // index of the chunk in progress
    uint32_t buf_len;    // bytes in buf
    uint32_t blocks;     // blocks of this chunk already compressed
    uint32_t depth;
    uint32_t stack[STACK][8];
    PM_HD void start_chunk() {
        for (int i = 0; i < 8; ++i) { cv[i] = B3Tables::IV[i]; buf[i] = 0; }
        buf_len = blocks = 0;
    }
    PM_HD void init() {
        chunk = 0;
        depth = 0;
        start_chunk();
    }
    PM_HD static void parent(const uint32_t l[8], const uint32_t r[8], bool root, uint32_t out[8]) {
        uint64_t blk[8];
        uint32_t iv[8];
        for (int i = 0; i < 4; ++i) {
            blk[i] = l[2 * i] | ((uint64_t)l[2 * i + 1] << 32);
            blk[4 + i] = r[2 * i] | ((uint64_t)r[2 * i + 1] << 32);
        }
        for (int i = 0; i < 8; ++i) iv[i] = B3Tables::IV[i];
        b3_compress(iv, blk, 0, 64, B3_PARENT | (root ? B3_ROOT : 0), out);
    }
    // the full block in buf, with more input behind it
    PM_HD void flush_block() {
        if (blocks == 15) {   // the chunk's last block: close the chunk, start the next
            b3_compress(cv, buf, chunk, 64, B3_CHUNK_END, cv);
            for (uint64_t t = chunk + 1; (t & 1) == 0; t >>= 1) {
                --depth;
                parent(stack[depth], cv, false, cv);
            }
            for (int i = 0; i < 8; ++i) stack[depth][i] = cv[i];
            ++depth;
            ++chunk;
            start_chunk();
            return;
        }
        b3_compress(cv, buf, chunk, 64, blocks == 0 ? B3_CHUNK_START : 0, cv);
        ++blocks;
        for (int i = 0; i < 8; ++i) buf[i] = 0;
        buf_len = 0;
    }
    PM_HD void absorb_le(uint64_t v, uint32_t n) {
        while (n) {
            if (buf_len == 64) flush_block();
            const uint32_t take = n < 64 - buf_len ? n : 64 - buf_len;
            xor_bytes_at(buf, buf_len, low_bytes(v, take), take);
            buf_len += take;
            v = take >= 8 ? 0 : v >> (8 * take);
            n -= take;
        }
    }
    PM_HD void absorb(const uint8_t *p, size_t n) { absorb_bytes(*this, p, n); }
    PM_HD void finish(uint64_t d[4]) {
        const uint32_t flags = (blocks == 0 ? B3_CHUNK_START : 0) | B3_CHUNK_END;
        b3_compress(cv, buf, chunk, buf_len, flags | (depth == 0 ? B3_ROOT : 0), cv);
        while (depth) {
            --depth;
            parent(stack[depth], cv, depth == 0, cv);
        }
        for (int i = 0; i < 4; ++i) d[i] = cv[2 * i] | ((uint64_t)cv[2 * i + 1] << 32);
    }
    PM_HD void finish(uint8_t out32[32]) {
        uint64_t d[4];
        finish(d);
        memcpy(out32, d, 32);
    }
};

// ------------------------------------------------------------------------------------------------------- STROBE-128 / Merlin
// hashes.hpp: Strobe128 (the part merlin uses).  cur_flags is only ever written there and is not kept.
struct Strobe128 {
    static constexpr uint32_t R = 166;
    uint64_t st[25];
    uint32_t pos, pos_begin;
    PM_HD void run_f() {
        xor_bytes_at(st, pos, pos_begin, 1);
        xor_bytes_at(st, pos + 1, 0x04, 1);
        xor_bytes_at(st, R + 1, 0x80, 1);
        keccak_f1600(st);
        pos = pos_begin = 0;
    }
    PM_HD void absorb_le(uint64_t v, uint32_t n) {
        while (n) {
            const uint32_t take = n < R - pos ? n : R - pos;
            xor_bytes_at(st, pos, low_bytes(v, take), take);
            pos += take;
            if (pos == R) run_f();
            v = take >= 8 ? 0 : v >> (8 * take);
            n -= take;
        }
    }
    PM_HD void begin_op(uint32_t flags) {   // `more` operations simply do not call it
        const uint64_t hdr = pos_begin | (flags << 8);
        pos_begin = pos + 1;
        absorb_le(hdr, 2);
        if ((flags & (4 | 32)) && pos != 0) run_f();
    }
    PM_HD void init(const uint8_t *label, size_t n) {
        for (int i = 0; i < 25; ++i) st[i] = 0;
        const uint8_t hdr[18] = {1, R + 2, 1, 0, 1, 96, 'S', 'T', 'R', 'O', 'B', 'E', 'v', '1', '.', '0', '.', '2'};
        st[0] = load_le(hdr, 8);
        st[1] = load_le(hdr + 8, 8);
        st[2] = load_le(hdr + 16, 2);
        keccak_f1600(st);
        pos = pos_begin = 0;
        meta_ad(label, n);
    }
    PM_HD void meta_ad(const uint8_t *d, size_t n) { begin_op(16 | 2); absorb_bytes(*this, d, n); }
    PM_HD void ad_begin() { begin_op(2); }
    // prf of 64 bytes: begin_op's C flag has run the permutation unless pos was 0, so the output starts at byte 0 and, being
    // shorter than the rate, meets no further permutation: 8 lanes read and cleared
    PM_HD void prf64(uint64_t out[8]) {
        begin_op(1 | 2 | 4);
        for (int i = 0; i < 8; ++i) { out[i] = st[i]; st[i] = 0; }
        pos = 64;
    }
};

// hashes.hpp: MerlinTranscript.  A message is begun with its total length and then absorbed piece by piece.
struct Merlin {
    Strobe128 s;
    PM_HD void init(const uint8_t *label, size_t n) {
        const uint8_t proto[11] = {'M', 'e', 'r', 'l', 'i', 'n', ' ', 'v', '1', '.', '0'}, dom[7] = {'d', 'o', 'm', '-', 's', 'e', 'p'};
        s.init(proto, 11);
        begin_message(dom, 7, (uint32_t)n);
        absorb_bytes(s, label, n);
    }
    PM_HD void begin_message(const uint8_t *label, size_t label_len, uint32_t msg_len) {
        s.meta_ad(label, label_len);
        s.absorb_le(msg_len, 4);   // meta_ad(LE32 length, more = true)
        s.ad_begin();
    }
    PM_HD void absorb_le(uint64_t v, uint32_t n) { s.absorb_le(v, n); }
    PM_HD void append_message(const uint8_t *label, size_t label_len, const uint8_t *msg, size_t n) {
        begin_message(label, label_len, (uint32_t)n);
        absorb_bytes(s, msg, n);
    }
    PM_HD void challenge_bytes64(const uint8_t *label, size_t label_len, uint64_t out[8]) {
        s.meta_ad(label, label_len);
        s.absorb_le(64, 4);
        s.prf64(out);
    }
};

// ------------------------------------------------------------------------------------------- transcript front ends, per kind
// host/polymath.hpp: MerlinFieldTranscript / HashTranscript.  begin_message(label, length of the message), then the pieces
// (put_le / put_bytes / put_fr), then challenge(label) -> Fr in Montgomery form.
template <class C>
PM_HD void fr_canonical_words(const Fp<typename C::FrP> &mont, uint64_t w[4]) {   // FrOps::to_le_bytes
    const Fp<typename C::FrP> c = from_mont<typename C::FrP>(mont);
    for (int i = 0; i < 4; ++i) w[i] = c.l[2 * i] | ((uint64_t)c.l[2 * i + 1] << 32);
}
template <class P>
PM_HD bool fr_words_canonical(const uint32_t l[8]) {   // < r, as FrOps::from_le_bytes_canonical / from_random_bytes decide it
    for (int i = 7; i >= 0; --i) {
        if (l[i] < P::MOD[i]) return true;
        if (l[i] > P::MOD[i]) return false;
    }
    return false;
}

template <class C, int KIND>
struct Transcript;

template <class C>
struct Transcript<C, KIND_MERLIN> {
    typedef typename C::FrP P;
    typedef Fp<P> Fr;
    Merlin m;
    PM_HD void init() {
        const uint8_t name[8] = {'p', 'o', 'l', 'y', 'm', 'a', 't', 'h'};
        m.init(name, 8);
    }
    PM_HD void begin_message(const uint8_t *label, size_t label_len, size_t msg_len) { m.begin_message(label, label_len, (uint32_t)msg_len); }
    PM_HD void put_le(uint64_t v, uint32_t n) { m.absorb_le(v, n); }
    // FrOps::from_random_bytes on 64 PRF bytes: the first 32 little-endian, masked to the modulus' bit length, drawn again while
    // >= r.  Each lane loops on its own draws: a wave is through when its last lane is.
    PM_HD Fr challenge(const uint8_t *label, size_t label_len) {
        constexpr int top_bits = P::BITS - 32 * 7;
        for (;;) {
            uint64_t buf[8];
            m.challenge_bytes64(label, label_len, buf);
            Fr v;
            for (int i = 0; i < 4; ++i) { v.l[2 * i] = (uint32_t)buf[i]; v.l[2 * i + 1] = (uint32_t)(buf[i] >> 32); }
            v.l[7] &= top_bits >= 32 ? 0xffffffffu : ((1u << top_bits) - 1);
            if (fr_words_canonical<P>(v.l)) return to_mont<P>(v);
        }
    }
};

template <class C, class H>
struct HashTranscriptT {
    typedef typename C::FrP P;
    typedef Fp<P> Fr;
    H h;   // the hash of the transcript bytes so far
    PM_HD void init() { h.init(); }
    PM_HD void begin_message(const uint8_t *label, size_t label_len, size_t) { absorb_bytes(h, label, label_len); }
    PM_HD void put_le(uint64_t v, uint32_t n) { h.absorb_le(v, n); }
    // the digest of (transcript || label) becomes the transcript; the challenge is F::from_be_bytes_mod_order of it
    PM_HD Fr challenge(const uint8_t *label, size_t label_len) {
        absorb_bytes(h, label, label_len);
        uint64_t d[4];
        h.finish(d);
        h.init();
        for (int i = 0; i < 4; ++i) h.absorb_le(d[i], 8);
        Fr v;
        for (int i = 0; i < 8; ++i) {   // 32-bit word i of the big-endian integer = bytes 28 - 4 i .. 31 - 4 i, reversed
            const uint32_t w = (uint32_t)(d[(7 - i) >> 1] >> (32 * ((7 - i) & 1)));
            v.l[i] = (w >> 24) | ((w >> 8) & 0xff00u) | ((w << 8) & 0xff0000u) | (w << 24);
        }
        return to_mont<P>(v);   // the Montgomery product reduces any 256-bit input mod r
    }
};
template <class C>
struct Transcript<C, KIND_KECCAK256> : HashTranscriptT<C, Keccak256Stream> {};
template <class C>
struct Transcript<C, KIND_BLAKE3> : HashTranscriptT<C, Blake3Stream> {};

template <class T>
PM_HD void put_bytes(T &t, const uint8_t *p, size_t n) {
    size_t i = 0;
    for (; i + 8 <= n; i += 8) t.put_le(load_le(p + i, 8), 8);
    if (i < n) t.put_le(load_le(p + i, (uint32_t)(n - i)), (uint32_t)(n - i));
}
template <class C, class T>
PM_HD void put_fr(T &t, const Fp<typename C::FrP> &mont) {
    uint64_t w[4];
    fr_canonical_words<C>(mont, w);
    for (int i = 0; i < 4; ++i) t.put_le(w[i], 8);
}

// ------------------------------------------------------------------------------------------------ the verifier's challenges
// The scalars of the verifying key the challenges need; n_inv = 1 / n, computed once per call.
template <class C>
struct FsVk {
    uint64_t n, sigma;
    Fp<typename C::FrP> omega, n_inv;
};
template <class C>
struct FsChallenges {
    Fp<typename C::FrP> x1, x2, c_at_x1;   // Montgomery
};

// sum_{i < 2 m0} z~_i l_i(x1), the part of compute_pi_at_x1 (common.rs:49-71, z~_i :77-97) before the factor y1^gamma, for
// pub = (1, inputs[0 .. n_inputs)), m0 = n_inputs + 1, with l_i(x1) = (x1^n - 1) / n * omega^i / (x1 - omega^i).
// The 2 m0 inverses are taken FS_INV_CHUNK at a time -- one Fermat inverse per chunk over the running product, Montgomery's
// trick; inverses are unique, so each equals the host's own -- and the first chunk also inverts `extra` (the verifier's y1).
// A term with x1 = omega^i, and a zero `extra`, get 0: what the host's a^(r-2) gives for 0.  Per-lane memory does not grow
// with m0: two arrays of FS_INV_CHUNK elements.
constexpr int FS_INV_CHUNK = 16;

template <class C>
PM_HD Fp<typename C::FrP> fs_lagrange_sum(const FsVk<C> &vk, const Fp<typename C::FrP> *inputs, size_t n_inputs, const Fp<typename C::FrP> &x1,
                                          const Fp<typename C::FrP> &extra, Fp<typename C::FrP> *extra_inv) {
    typedef typename C::FrP P;
    typedef Fp<P> Fr;
    const size_t m0 = n_inputs + 1, total = 2 * m0;
    const Fr one = Fr::one();
    Fr sum = Fr::zero(), w = one;
    Fr num = mul<P>(sub<P>(pow_u64<P>(x1, vk.n), one), vk.n_inv);
    Fr diff[FS_INV_CHUNK], pre[FS_INV_CHUNK];
#pragma unroll 1
    for (size_t base = 0; base < total; base += FS_INV_CHUNK) {
        const int cnt = (int)(total - base < (size_t)FS_INV_CHUNK ? total - base : (size_t)FS_INV_CHUNK);
        Fr acc = base == 0 && !extra.is_zero() ? extra : one;
#pragma unroll 1
        for (int j = 0; j < cnt; ++j) {   // pre[j]: the product of the non-zero terms before term j
            const Fr d = sub<P>(x1, w);
            diff[j] = d;
            pre[j] = acc;
            if (!d.is_zero()) acc = mul<P>(acc, d);
            w = mul<P>(w, vk.omega);
        }
        Fr inv = inverse<P>(acc);   // acc != 0
#pragma unroll 1
        for (int j = cnt - 1; j >= 0; --j) {   // pre[j] becomes 1 / diff[j]
            const Fr d = diff[j];
            if (d.is_zero()) { pre[j] = Fr::zero(); continue; }
            pre[j] = mul<P>(inv, pre[j]);
            inv = mul<P>(inv, d);
        }
        if (base == 0) *extra_inv = extra.is_zero() ? Fr::zero() : inv;
#pragma unroll 1
        for (int j = 0; j < cnt; ++j) {
            const size_t i = base + j;
            const Fr zt = i == 0 ? add<P>(one, one) : i < m0 ? add<P>(one, inputs[i - 1]) : i == m0 ? Fr::zero() : sub<P>(one, inputs[i - m0 - 1]);
            sum = add<P>(sum, mul<P>(zt, mul<P>(num, pre[j])));
            num = mul<P>(num, vk.omega);
        }
    }
    return sum;
}

// The two halves of the transcript that the prover and the verifier share (common.rs:21-37), on a transcript the caller owns:
// fs_absorb_x1 starts it (prover.rs:125 / verifier.rs:24), hashes the public inputs -- `first` and then inputs[0 .. n_inputs): the
// verifier's `first` is one, the prover's is element 0 of its instance -- and the compressed records of [a]_1 and [c]_1 (4 * C::FqP::N
// bytes each), and draws x1; fs_absorb_x2 continues the same transcript with x1, a(x1), c(x1) and draws x2.
template <class C, class T>
PM_HD Fp<typename C::FrP> fs_absorb_x1(T &t, const Fp<typename C::FrP> &first, const Fp<typename C::FrP> *inputs, size_t n_inputs, const uint8_t *a_rec,
                                       const uint8_t *c_rec) {
    constexpr size_t NB = 4 * C::FqP::N;
    const uint8_t l_pub[13] = {'p', 'u', 'b', 'l', 'i', 'c', '_', 'i', 'n', 'p', 'u', 't', 's'};
    const uint8_t l_com[11] = {'c', 'o', 'm', 'm', 'i', 't', 'm', 'e', 'n', 't', 's'}, l_x1[2] = {'x', '1'};
    t.init();
    const size_t m0 = n_inputs + 1;
    t.begin_message(l_pub, 13, 8 + 32 * m0);                            // common.rs:21-30
    t.put_le(m0, 8);
    put_fr<C>(t, first);
    for (size_t i = 0; i < n_inputs; ++i) put_fr<C>(t, inputs[i]);
    t.begin_message(l_com, 11, 8 + 2 * NB);
    t.put_le(2, 8);
    put_bytes(t, a_rec, NB);
    put_bytes(t, c_rec, NB);
    return t.challenge(l_x1, 2);
}
template <class C, class T>
PM_HD Fp<typename C::FrP> fs_absorb_x2(T &t, const Fp<typename C::FrP> &x1, const Fp<typename C::FrP> &a_at_x1, const Fp<typename C::FrP> &c_at_x1) {
    const uint8_t l_val[6] = {'v', 'a', 'l', 'u', 'e', 's'}, l_x1[2] = {'x', '1'}, l_x2[2] = {'x', '2'};
    t.begin_message(l_x1, 2, 32);                                       // common.rs:32-37
    put_fr<C>(t, x1);
    t.begin_message(l_val, 6, 8 + 64);
    t.put_le(2, 8);
    put_fr<C>(t, a_at_x1);
    put_fr<C>(t, c_at_x1);
    return t.challenge(l_x2, 2);
}
// c(x1) of common.rs:73-75 from a(x1), y1^gamma, pi(x1) and y1: 1 / y1^alpha is y1^3 (alpha = -3), no inversion; 0 for y1 = 0, which is
// what the host's a^(r-2) gives for 1 / 0
template <class P>
PM_HD Fp<P> fs_c_at_x1(const Fp<P> &a_at, const Fp<P> &y1_gamma, const Fp<P> &pi_at_x1, const Fp<P> &y1) {
    const Fp<P> y1_alpha_inv = mul<P>(sqr<P>(y1), y1);
    return mul<P>(sub<P>(mul<P>(add<P>(a_at, y1_gamma), a_at), pi_at_x1), y1_alpha_inv);
}

// Polymath::verifier_challenges (host/polymath.hpp; verifier.rs:24-42) for one proof: a_rec / c_rec are the compressed records of
// [a]_1 and [c]_1 (4 * C::FqP::N bytes each, hashed as they arrived), a_at_x1_bytes the 32 little-endian bytes of a(x1), inputs
// the public inputs without the leading one (Montgomery).  false, nothing computed, when a_at_x1 >= r (what
// FrOps::from_le_bytes_canonical refuses).  1 / y1 comes out of the Lagrange sum's first chunk.
template <class C, int KIND>
PM_HD bool fs_verifier_challenges(const FsVk<C> &vk, const Fp<typename C::FrP> *inputs, size_t n_inputs, const uint8_t *a_rec, const uint8_t *c_rec,
                                  const uint8_t *a_at_x1_bytes, FsChallenges<C> *out, Fp<typename C::FrP> *a_at_x1_out) {
    typedef typename C::FrP P;
    typedef Fp<P> Fr;
    Fr a_at;
    for (int i = 0; i < 4; ++i) {
        const uint64_t v = load_le(a_at_x1_bytes + 8 * i, 8);
        a_at.l[2 * i] = (uint32_t)v;
        a_at.l[2 * i + 1] = (uint32_t)(v >> 32);
    }
    if (!fr_words_canonical<P>(a_at.l)) return false;
    a_at = to_mont<P>(a_at);
    *a_at_x1_out = a_at;

    Transcript<C, KIND> t;
    const Fr x1 = fs_absorb_x1<C>(t, Fr::one(), inputs, n_inputs, a_rec, c_rec);   // verifier.rs:24-29
    const Fr y1 = pow_u64<P>(x1, vk.sigma);                             // verifier.rs:32
    Fr y1_inv;
    const Fr lag = fs_lagrange_sum<C>(vk, inputs, n_inputs, x1, y1, &y1_inv);
    const Fr y1_gamma = pow_u64<P>(y1_inv, 5);                          // :34, MINUS_GAMMA
    const Fr pi_at_x1 = mul<P>(lag, y1_gamma);                          // :35
    const Fr c_at_x1 = fs_c_at_x1<P>(a_at, y1_gamma, pi_at_x1, y1);     // :37-40
    out->x1 = x1;
    out->c_at_x1 = c_at_x1;
    out->x2 = fs_absorb_x2<C>(t, x1, a_at, c_at_x1);                    // verifier.rs:42
    return true;
}

// ------------------------------------------------------------------------------------------------ the prover's challenges
// Polymath::glue_x1 / glue_x2 (host/polymath.hpp; prover.rs:125-138, 189) for one proof, in two halves because phase 2 runs between
// them.  What the first half hands to the second is this record, the transcript included: the sponge is STORED (208 bytes for Merlin
// and Keccak-256, 888 for BLAKE3), not rebuilt -- rebuilding would hash the 32 m0 + 2 * 48 bytes of the first two messages a second
// time, which grows with m0, while the record is a fixed few hundred bytes a proof beside vectors of 23 n field elements.
template <class C, int KIND>
struct FsProverState {
    Transcript<C, KIND> t;
    Fp<typename C::FrP> x1, y1_alpha, y1_gamma;   // Montgomery; y1_alpha = y1^alpha = 1 / y1^3, y1_gamma = 1 / y1^5
};
template <class C>
struct FsProverOut {
    Fp<typename C::FrP> a_at_x1, pi_at_x1, c_at_x1, x2;
};

// instance: the m0 hashed public inputs, element 0 (the constant one of a well-formed assignment) included, as the host hashes them.
// ONE inversion, of y1 = x1^sigma (0 for y1 = 0, as the host's); its third and fifth powers.
template <class C, int KIND>
PM_HD void fs_prover_x1(const FsVk<C> &vk, const Fp<typename C::FrP> *instance, size_t m0, const uint8_t *a_rec, const uint8_t *c_rec,
                        FsProverState<C, KIND> *s) {
    typedef typename C::FrP P;
    typedef Fp<P> Fr;
    s->x1 = fs_absorb_x1<C>(s->t, instance[0], instance + 1, m0 - 1, a_rec, c_rec);   // prover.rs:125-126
    const Fr y1_inv = inverse<P>(pow_u64<P>(s->x1, vk.sigma));         // :128
    s->y1_alpha = pow_u64<P>(y1_inv, 3);                                // :130, MINUS_ALPHA
    s->y1_gamma = pow_u64<P>(y1_inv, 5);                                // :134, MINUS_GAMMA
}
// u_at_x1: phase 2's u(x1); r_a: the proof's two blinding coefficients, constant term first
template <class C, int KIND>
PM_HD void fs_prover_x2(const FsVk<C> &vk, const Fp<typename C::FrP> *instance, size_t m0, FsProverState<C, KIND> *s, const Fp<typename C::FrP> &u_at_x1,
                        const Fp<typename C::FrP> r_a[2], FsProverOut<C> *out) {
    typedef typename C::FrP P;
    typedef Fp<P> Fr;
    const Fr ra_at = add<P>(r_a[0], mul<P>(r_a[1], s->x1));
    out->a_at_x1 = add<P>(u_at_x1, mul<P>(ra_at, s->y1_alpha));         // prover.rs:132
    Fr none;
    out->pi_at_x1 = mul<P>(fs_lagrange_sum<C>(vk, instance + 1, m0 - 1, s->x1, Fr::zero(), &none), s->y1_gamma);   // :135
    out->c_at_x1 = fs_c_at_x1<P>(out->a_at_x1, s->y1_gamma, out->pi_at_x1, pow_u64<P>(s->x1, vk.sigma));          // :138
    out->x2 = fs_absorb_x2<C>(s->t, s->x1, out->a_at_x1, out->c_at_x1);                                           // :189
}

}  // namespace fs
}  // namespace pm
