// ark-serialize's compressed record of one G1 point as PM_HD code (host/wire.hpp: ser_g1 is the specification): the text of
// k_g1_encode (g1_codec.hip: exported keys) and of the batch prover's glue kernels (prove_glue.hip: the records the transcript hashes
// and the proof's bytes).  BLS12-381: 48 bytes, x big-endian, flags in the first byte (0x80 compressed, 0x40 infinity, 0x20 y > -y);
// BN254: 32 bytes, x little-endian, flags in the last byte (0x80 y > -y, 0x40 infinity).
#pragma once
#include "ec.cuh"

namespace pm {

// canonical a > (p - 1) / 2, i.e. a > -a in the integer order deser_g1 compares in (fq_cmp(y, -y) > 0)
template <class P>
PM_HD bool fq_canon_gt_half(const Fp<P> &a) {
    bool gt = false, decided = false;
#pragma unroll
    for (int i = P::N - 1; i >= 0; --i) {
        const uint32_t h = (P::MOD[i] >> 1) | (i + 1 < P::N ? P::MOD[i + 1] << 31 : 0u);
        if (!decided && a.l[i] != h) { gt = a.l[i] > h; decided = true; }
    }
    return gt;
}

PM_HD uint32_t bswap32(uint32_t v) { return __builtin_bswap32(v); }

// w[0 .. C::FqP::N): the record of the standard-Montgomery affine point `a` as little-endian 32-bit words of its byte string; with
// `inf` the coordinates are not read
template <class C>
PM_HD void g1_record_words(const Affine<C> &a, bool inf, uint32_t *w) {
    typedef typename C::FqP P;
    constexpr int NW = P::N;
    const Fp<P> x = inf ? Fp<P>::zero() : from_mont<P>(a.x);
    const bool larger = !inf && fq_canon_gt_half<P>(from_mont<P>(a.y));
    if (C::ID == 0) {
#pragma unroll
        for (int k = 0; k < NW; ++k) w[k] = bswap32(x.l[NW - 1 - k]);
        w[0] |= 0x80u | (inf ? 0x40u : 0u) | (larger ? 0x20u : 0u);
    } else {
#pragma unroll
        for (int k = 0; k < NW; ++k) w[k] = x.l[k];
        w[NW - 1] |= ((inf ? 0x40u : 0u) | (larger ? 0x80u : 0u)) << 24;
    }
}

}  // namespace pm
