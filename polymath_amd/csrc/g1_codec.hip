// G1 point records on the device, compressed (below) and uncompressed (k_g1_decode_uncompressed / k_g1_encode_uncompressed).
// Compressed G1 points: ProvingKey::serialize_compressed (data_structures.rs:56-73) holds every base as
// ark-serialize's compressed encoding, and a key from somebody else's setup arrives as exactly that.  Decoding costs one
// square root in Fq per point (and, under Validate::Yes, a subgroup check on BLS12-381): ~4 400 Fq products a point, 26 M
// points at 2^20 gates -- hours on one host thread, about a second here.  The host mirror polymath_amd/host/wire.hpp
// (deser_g1, ser_g1, g1_in_subgroup) is the bit-exact specification of both kernels.
//
// One lane per point.  Flags, infinity and malformed input are MASKED, not branched on: a lane whose encoding has already
// failed (or is the point at infinity) runs the same square-root chain and subgroup loop on a dummy value and drops the
// result, so the exponent chain and the scalar loop stay wave-uniform.
#include <algorithm>
#include <cstring>

#include "internal.h"
#include "g1_record.cuh"
#include "../host/wire.hpp"

namespace pm {

// canonical a < p
template <class P>
__device__ __forceinline__ bool fq_canon_lt_p(const Fp<P> &a) {
    bool lt = false, decided = false;
#pragma unroll
    for (int i = P::N - 1; i >= 0; --i)
        if (!decided && a.l[i] != P::MOD[i]) { lt = a.l[i] < P::MOD[i]; decided = true; }
    return lt;
}

// a^((p+1)/4): the square root when one exists (p = 3 mod 4 on both curves; p + 1 does not carry out of limb 0).  The exponent
// is a constant: its bits are the same on every lane, so the branch below is a scalar one.
template <class P>
__device__ Fp<P> fq_pow_p1_4(const Fp<P> &a) {
    Fp<P> acc = Fp<P>::one();
#pragma unroll 1
    for (int i = P::N - 1; i >= 0; --i) {
        const uint32_t lo = P::MOD[i] + (i == 0 ? 1u : 0u), hi = i + 1 < P::N ? P::MOD[i + 1] : 0u;
        const uint32_t e = (lo >> 2) | (hi << 30);
#pragma unroll 1
        for (int b = 31; b >= 0; --b) {
            acc = sqr<P>(acc);
            if ((e >> b) & 1u) acc = mul<P>(acc, a);
        }
    }
    return acc;
}

// [r] P == O (g1_in_subgroup of wire.hpp, the same double-and-add over the bits of r): P affine, Montgomery, not infinity
template <class C>
__device__ bool g1_r_torsion(const Affine<C> &p) {
    return xyzz_mul_words<C>(p, C::FrP::MOD, C::FrP::N).is_identity();
}

template <class C>
__global__ __launch_bounds__(256, 2) void k_g1_decode(const uint8_t *in, size_t count, int validate, Affine<C> *out, uint8_t *status,
                                                   unsigned long long *first_bad, uint64_t base_index) {
    typedef typename C::FqP P;
    typedef Fp<P> Fq;
    constexpr int NW = P::N, NB = 4 * NW;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    uint32_t w[NW];
    const uint4 *src = (const uint4 *)(in + i * NB);   // NB = 48 / 32 and a 16-byte aligned base: whole 16-byte loads
#pragma unroll
    for (int k = 0; k < NB / 16; ++k) {
        const uint4 v = src[k];
        w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w;
    }
    Fq x;
    bool inf, larger;
    int st = PM_G1_OK;
    if (C::ID == 0) {   // zcash: big-endian, flags in the first byte
        const uint32_t flags = w[0] & 0xFFu;
#pragma unroll
        for (int k = 0; k < NW; ++k) x.l[k] = __builtin_bswap32(w[NW - 1 - k]);
        x.l[NW - 1] &= 0x1FFFFFFFu;
        inf = (flags & 0x40u) != 0;
        larger = (flags & 0x20u) != 0;
        if (!(flags & 0x80u)) st = PM_G1_BAD_FLAGS;
        else if (inf && larger) st = PM_G1_INF_SIGN;
    } else {            // ark short Weierstrass: little-endian, flags in the last byte
        const uint32_t flags = w[NW - 1] >> 24;
#pragma unroll
        for (int k = 0; k < NW; ++k) x.l[k] = w[k];
        x.l[NW - 1] &= 0x3FFFFFFFu;
        inf = (flags & 0x40u) != 0;
        larger = (flags & 0x80u) != 0;
        if (inf && larger) st = PM_G1_BAD_FLAGS;
    }
    if (st == PM_G1_OK && inf && !x.is_zero()) st = PM_G1_NONCANONICAL_INF;
    if (st == PM_G1_OK && !inf && !fq_canon_lt_p<P>(x)) st = PM_G1_COORD_GE_P;
    const bool live = st == PM_G1_OK && !inf;          // lanes that decode a real point; the others compute on x = 0
    Fq b;
#pragma unroll
    for (int k = 0; k < NW; ++k) b.l[k] = C::B_MONT[k];
    const Fq xm = live ? to_mont<P>(x) : Fq::zero();
    const Fq rhs = add<P>(mul<P>(sqr<P>(xm), xm), b);
    Fq y = fq_pow_p1_4<P>(rhs);
    if (live && !sqr<P>(y).eq(rhs)) st = PM_G1_NOT_ON_CURVE;
    if (fq_canon_gt_half<P>(from_mont<P>(y)) != larger) y = neg<P>(y);
    Affine<C> pt{xm, y};
    if (C::ID == 0 && validate) {                      // BN254's G1 has cofactor 1: nothing to check there
        Affine<C> probe = pt;
        if (!(live && st == PM_G1_OK)) {               // masked lane: the generator stands in
#pragma unroll
            for (int k = 0; k < NW; ++k) { probe.x.l[k] = C::GX_MONT[k]; probe.y.l[k] = C::GY_MONT[k]; }
        }
        const bool in_g1 = g1_r_torsion<C>(probe);
        if (live && st == PM_G1_OK && !in_g1) st = PM_G1_NOT_IN_SUBGROUP;
    }
    if (st != PM_G1_OK || inf) pt = Affine<C>::infinity();   // the ABI's infinity: x = y = 0
    out[i] = pt;
    if (status) status[i] = (uint8_t)st;
    if (st != PM_G1_OK && first_bad) atomicMin(first_bad, (unsigned long long)(((base_index + i) << 8) | (uint64_t)st));
}

template <class C>
__global__ __launch_bounds__(256) void k_g1_encode(const Affine<C> *pts, size_t count, uint8_t *out) {
    constexpr int NW = C::FqP::N, NB = 4 * NW;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const Affine<C> a = pts[i];
    uint32_t w[NW];
    g1_record_words<C>(a, a.is_inf(), w);
    uint4 *dst = (uint4 *)(out + i * NB);
#pragma unroll
    for (int k = 0; k < NB / 16; ++k) dst[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
}

// The uncompressed record (ser_g1_uncompressed / deser_g1_uncompressed of wire.hpp): x || y, 96 / 64 bytes, read as whole 16-byte
// words.  No square root: the pair is checked against the curve equation (always) and, under validate, against the subgroup.  The
// same masking as k_g1_decode: a lane whose record is refused or is infinity computes on x = y = 0 and, in the subgroup loop, on the
// generator; it writes the same Affine<C> (standard Montgomery; refused and infinity x = y = 0), so nothing downstream can tell the
// two forms apart.  SUBGROUP (validate on BLS12-381) is a template argument: without it the kernel is five products beside a copy, and
// must not carry the scalar loop's registers and scratch (248 VGPRs, 2 waves a SIMD) through what is then a memory-bound pass.
template <class C, bool SUBGROUP>
__global__ __launch_bounds__(256, SUBGROUP ? 2 : 4) void k_g1_decode_uncompressed(const uint8_t *in, size_t count, Affine<C> *out, uint8_t *status,
                                                                               unsigned long long *first_bad, uint64_t base_index) {
    typedef typename C::FqP P;
    typedef Fp<P> Fq;
    constexpr int NW = P::N, NB = 8 * NW;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    uint32_t w[2 * NW];
    const uint4 *src = (const uint4 *)(in + i * NB);   // NB = 96 / 64 and a 16-byte aligned base: whole 16-byte loads
#pragma unroll
    for (int k = 0; k < NB / 16; ++k) {
        const uint4 v = src[k];
        w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w;
    }
    Fq x, y;
    bool inf;
    int st = PM_G1_OK;
    if (C::ID == 0) {   // zcash: big-endian, flags in the first byte -- x's top three bits; y uses all of its 384
        const uint32_t flags = w[0] & 0xFFu;
#pragma unroll
        for (int k = 0; k < NW; ++k) { x.l[k] = __builtin_bswap32(w[NW - 1 - k]); y.l[k] = __builtin_bswap32(w[2 * NW - 1 - k]); }
        x.l[NW - 1] &= 0x1FFFFFFFu;
        inf = (flags & 0x40u) != 0;
        if (flags & 0x80u) st = PM_G1_BAD_FLAGS;                       // a compressed record
        else if (flags & 0x20u) st = inf ? PM_G1_INF_SIGN : PM_G1_BAD_FLAGS;   // the sort bit belongs to the compressed form
    } else {            // ark short Weierstrass: little-endian, flags in the last byte -- y's top two bits; x carries none
        const uint32_t flags = w[2 * NW - 1] >> 24;
#pragma unroll
        for (int k = 0; k < NW; ++k) { x.l[k] = w[k]; y.l[k] = w[NW + k]; }
        y.l[NW - 1] &= 0x3FFFFFFFu;
        inf = (flags & 0x40u) != 0;
        if (inf && (flags & 0x80u)) st = PM_G1_BAD_FLAGS;              // 0x80 on a finite point ("y > -y") is not read
    }
    if (st == PM_G1_OK && inf && !(x.is_zero() && y.is_zero())) st = PM_G1_NONCANONICAL_INF;
    if (st == PM_G1_OK && !inf && !(fq_canon_lt_p<P>(x) && fq_canon_lt_p<P>(y))) st = PM_G1_COORD_GE_P;
    const bool live = st == PM_G1_OK && !inf;          // lanes that hold a real pair; the others compute on x = y = 0
    Fq b;
#pragma unroll
    for (int k = 0; k < NW; ++k) b.l[k] = C::B_MONT[k];
    const Fq xm = live ? to_mont<P>(x) : Fq::zero(), ym = live ? to_mont<P>(y) : Fq::zero();
    if (live && !sqr<P>(ym).eq(add<P>(mul<P>(sqr<P>(xm), xm), b))) st = PM_G1_NOT_ON_CURVE;   // always: validate adds the subgroup only
    Affine<C> pt{xm, ym};
    if (SUBGROUP) {                                    // BN254's G1 has cofactor 1: nothing to check there
        Affine<C> probe = pt;
        if (!(live && st == PM_G1_OK)) {               // masked lane: the generator stands in
#pragma unroll
            for (int k = 0; k < NW; ++k) { probe.x.l[k] = C::GX_MONT[k]; probe.y.l[k] = C::GY_MONT[k]; }
        }
        const bool in_g1 = g1_r_torsion<C>(probe);
        if (live && st == PM_G1_OK && !in_g1) st = PM_G1_NOT_IN_SUBGROUP;
    }
    if (st != PM_G1_OK || inf) pt = Affine<C>::infinity();   // the ABI's infinity: x = y = 0
    out[i] = pt;
    if (status) status[i] = (uint8_t)st;
    if (st != PM_G1_OK && first_bad) atomicMin(first_bad, (unsigned long long)(((base_index + i) << 8) | (uint64_t)st));
}

template <class C>
__global__ __launch_bounds__(256) void k_g1_encode_uncompressed(const Affine<C> *pts, size_t count, uint8_t *out) {
    typedef typename C::FqP P;
    constexpr int NW = P::N, NB = 8 * NW;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const Affine<C> a = pts[i];
    const bool inf = a.is_inf();
    const Fp<P> x = inf ? Fp<P>::zero() : from_mont<P>(a.x), y = inf ? Fp<P>::zero() : from_mont<P>(a.y);
    uint32_t w[2 * NW];
    if (C::ID == 0) {
#pragma unroll
        for (int k = 0; k < NW; ++k) { w[k] = __builtin_bswap32(x.l[NW - 1 - k]); w[NW + k] = __builtin_bswap32(y.l[NW - 1 - k]); }
        w[0] |= inf ? 0x40u : 0u;
    } else {
#pragma unroll
        for (int k = 0; k < NW; ++k) { w[k] = x.l[k]; w[NW + k] = y.l[k]; }
        w[2 * NW - 1] |= (inf ? 0x40u : (fq_canon_gt_half<P>(y) ? 0x80u : 0u)) << 24;
    }
    uint4 *dst = (uint4 *)(out + i * NB);
#pragma unroll
    for (int k = 0; k < NB / 16; ++k) dst[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
}

template <class C>
int g1_decode_device(pm_ctx *ctx, const uint8_t *d_in, size_t count, bool validate, Affine<C> *d_out, uint8_t *d_status,
                     unsigned long long *d_first_bad, uint64_t base_index, int form) {
    if (!count) return PM_OK;
    if (((uintptr_t)d_in & 15) != 0) { ctx->err = "g1_decode: staging not 16-byte aligned"; return PM_ERR_STATE; }
    const dim3 grid((unsigned)((count + 255) / 256));
    if (form == PM_WIRE_UNCOMPRESSED && validate)      // BN254: the same kernel either way
        PM_LAUNCH(ctx, (k_g1_decode_uncompressed<C, C::ID == 0>), grid, dim3(256), 0, ctx->stream, d_in, count, d_out, d_status, d_first_bad, base_index);
    else if (form == PM_WIRE_UNCOMPRESSED)
        PM_LAUNCH(ctx, (k_g1_decode_uncompressed<C, false>), grid, dim3(256), 0, ctx->stream, d_in, count, d_out, d_status, d_first_bad, base_index);
    else
        PM_LAUNCH(ctx, k_g1_decode<C>, grid, dim3(256), 0, ctx->stream, d_in, count, validate ? 1 : 0, d_out, d_status, d_first_bad, base_index);
    return PM_OK;
}

template <class C>
int g1_encode_device(pm_ctx *ctx, const Affine<C> *d_pts, size_t count, uint8_t *d_out, int form) {
    if (!count) return PM_OK;
    if (((uintptr_t)d_out & 15) != 0) { ctx->err = "g1_encode: staging not 16-byte aligned"; return PM_ERR_STATE; }
    const dim3 grid((unsigned)((count + 255) / 256));
    if (form == PM_WIRE_UNCOMPRESSED) PM_LAUNCH(ctx, k_g1_encode_uncompressed<C>, grid, dim3(256), 0, ctx->stream, d_pts, count, d_out);
    else PM_LAUNCH(ctx, k_g1_encode<C>, grid, dim3(256), 0, ctx->stream, d_pts, count, d_out);
    return PM_OK;
}

const char *g1_status_text(int curve, int status, int form) {
    switch (status) {
    case PM_G1_OK: return "ok";
    case PM_G1_BAD_FLAGS:
        if (curve != PM_BLS12_381) return "G1: both flag bits set";
        return form == PM_WIRE_UNCOMPRESSED ? "G1: not an uncompressed point" : "G1: not a compressed point";
    case PM_G1_COORD_GE_P: return "G1: coordinate >= p";
    case PM_G1_NOT_ON_CURVE: return "G1: not on the curve";
    case PM_G1_NOT_IN_SUBGROUP: return "G1: not in the prime-order subgroup";
    case PM_G1_NONCANONICAL_INF: return "G1: non-canonical encoding of the point at infinity";
    case PM_G1_INF_SIGN: return "G1: sign bit on the point at infinity";
    default: return "G1: unknown status";
    }
}

// The key's byte string parsed as far as the host needs it: vk (points validated: four of them), the SAP header and matrices,
// and where each base vector's point records start.  The points themselves are left to the decode kernels.  `form` (pm_wire_form)
// gives the record size and the vk reader; bytes of the other form fail here, as a malformed key.
template <class C>
int pk_wire_parse(const uint8_t *data, size_t len, int form, WireLayout &out, std::string &err) {
    const size_t NB = g1_record_bytes<C>(form);
    try {
        pmhost::Reader rd(data, len);
        const pmhost::VerifyingKeyT<C> vk = pmhost::read_vk_c<C>(rd, form);
        out.vk_len = rd.off;
        out.n = vk.n; out.vk_m0 = vk.m0; out.sigma = vk.sigma;
        memcpy(out.omega, vk.omega.l, 32);
        constexpr int NQ = C::FqP::N;
        if (!vk.one_g1.inf) { memcpy(out.vk_one_g1, vk.one_g1.p.x.l, 4 * NQ); memcpy(out.vk_one_g1 + NQ, vk.one_g1.p.y.l, 4 * NQ); }
        const typename pmhost::PairingOf<C>::type::G2 *q[3] = {&vk.one_g2, &vk.x_g2, &vk.z_g2};
        for (int j = 0; j < 3; ++j) {
            if (q[j]->inf) { out.vk_g2_inf = true; continue; }
            uint32_t *g = out.vk_g2 + j * 4 * NQ;
            memcpy(g, q[j]->x.c0.l, 4 * NQ); memcpy(g + NQ, q[j]->x.c1.l, 4 * NQ);
            memcpy(g + 2 * NQ, q[j]->y.c0.l, 4 * NQ); memcpy(g + 3 * NQ, q[j]->y.c1.l, 4 * NQ);
        }
        out.m0 = rd.u64(); out.mw = rd.u64(); out.nr = rd.u64();
        for (int k = 0; k < 3; ++k) {
            pmhost::CsrHost m = pmhost::WireKey<C>::get_matrix(rd);
            out.rowptr[k] = std::move(m.rowptr);
            out.col[k] = std::move(m.col);
            out.val[k] = std::move(m.val);
        }
        for (int which : pmhost::PK_WIRE_VECTORS) {
            const uint64_t cnt = rd.u64();
            if (cnt > (len - rd.off) / NB) throw pmhost::WireError("truncated key");
            out.vec_len[which] = cnt;
            out.vec_off[which] = rd.off;
            rd.off += cnt * NB;
        }
        if (rd.off != len) throw pmhost::WireError("trailing bytes after the key");
    } catch (const std::exception &e) {
        err = std::string("pm_pk_load_bytes: ") + e.what();
        return PM_ERR_INVALID_ARG;
    }
    return PM_OK;
}

#define PM_INST(C)                                                                                                              \
    template int g1_decode_device<C>(pm_ctx *, const uint8_t *, size_t, bool, Affine<C> *, uint8_t *, unsigned long long *, uint64_t, int); \
    template int g1_encode_device<C>(pm_ctx *, const Affine<C> *, size_t, uint8_t *, int);                                     \
    template int pk_wire_parse<C>(const uint8_t *, size_t, int, WireLayout &, std::string &);
PM_INST(BlsCurve)
PM_INST(BnCurve)

}  // namespace pm
