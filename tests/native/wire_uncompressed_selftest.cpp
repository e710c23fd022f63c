// CPU-only test of the uncompressed wire form (polymath_amd/host/wire.hpp: ser_g1_uncompressed, deser_g1_uncompressed, the G2 pair,
// the vk and WireKey readers and writers with a form): no GPU, no library link.  argv = files holding the hex of a serialised
// ProvingKey (tests/golden/pk_wire.json).  Expected bytes are the literals of the format's description; expected texts are the
// compressed form's except "G1: not an uncompressed point".
#include <cstdio>
#include <fstream>
#include <string>
#include "../../polymath_amd/host/wire.hpp"
using namespace pmhost;

static int fails = 0, checks = 0;
static void check(bool ok, const char *curve, const std::string &what) {
    ++checks;
    if (!ok) { ++fails; printf("%s: FAILED %s\n", curve, what.c_str()); }
}

static Bytes unhex(const std::string &s) {
    Bytes b;
    auto nib = [](char ch) { return ch <= '9' ? ch - '0' : (ch | 32) - 'a' + 10; };
    for (size_t i = 0; i + 1 < s.size(); i += 2) b.push_back((uint8_t)(nib(s[i]) << 4 | nib(s[i + 1])));
    return b;
}

// the text deser_g1_uncompressed refuses `rec` with; "" when it accepts
template <class C>
static std::string refusal(const Bytes &rec, bool validate) {
    try {
        Reader rd(rec.data(), rec.size());
        deser_g1_uncompressed<C>(rd, validate);
    } catch (const WireError &e) { return e.what(); }
    return "";
}

template <class C>
static G1Point<C> generator() {
    G1Point<C> g;
    for (int i = 0; i < C::FqP::N; ++i) { g.p.x.l[i] = C::GX_MONT[i]; g.p.y.l[i] = C::GY_MONT[i]; }
    g.inf = false;
    return g;
}

template <class C>
static bool same(const G1Point<C> &a, const G1Point<C> &b) {
    return a.inf == b.inf && (a.inf || (a.p.x.eq(b.p.x) && a.p.y.eq(b.p.y)));
}

// canonical integer (little-endian limbs) -> the coordinate's bytes in the curve's byte order
template <class C>
static Bytes coord_bytes(const uint32_t *limbs) {
    const int NB = 4 * C::FqP::N;
    Bytes le((const uint8_t *)limbs, (const uint8_t *)limbs + NB);
    if (C::ID == 0) return Bytes(le.rbegin(), le.rend());
    return le;
}
template <class C>
static void put_coord(Bytes &rec, int half, const uint32_t *limbs) {
    const int NB = 4 * C::FqP::N;
    const Bytes b = coord_bytes<C>(limbs);
    std::copy(b.begin(), b.end(), rec.begin() + half * NB);
}

template <class C>
static void run(const char *curve, const std::string &gen_hex, const std::string &inf_hex, size_t vk_c, size_t vk_u) {
    typedef typename C::FqP Q;
    typedef typename PairingOf<C>::type B;
    const int NW = Q::N, NB = 4 * NW;
    const bool bls = C::ID == 0;
    const int flag_at = bls ? 0 : 2 * NB - 1;
    const G1Point<C> G = generator<C>();
    G1Point<C> O;
    memset(&O.p, 0, sizeof(O.p));
    O.inf = true;

    // ---- the four literals, both ways
    Bytes gen, inf;
    ser_g1_uncompressed<C>(G, gen);
    ser_g1_uncompressed<C>(O, inf);
    check(to_hex(gen) == gen_hex, curve, "generator bytes");
    check(to_hex(inf) == inf_hex, curve, "infinity bytes");
    {
        const Bytes a = unhex(gen_hex), b = unhex(inf_hex);
        Reader ra(a.data(), a.size()), rb(b.data(), b.size());
        check(same<C>(deser_g1_uncompressed<C>(ra), G) && ra.off == (size_t)2 * NB, curve, "generator decode");
        check(deser_g1_uncompressed<C>(rb).inf && rb.off == (size_t)2 * NB, curve, "infinity decode");
    }

    // ---- k G, k = 1 .. 64: both forms decode to the same point, and (x, -y) too
    pm::XYZZ<C> acc = pm::XYZZ<C>::identity();
    for (int k = 1; k <= 64; ++k) {
        pm::xyzz_madd<C>(acc, G.p, false);
        for (int sign = 0; sign < 2; ++sign) {
            G1Point<C> P{pm::xyzz_to_affine<C>(acc), false};
            if (sign) P.p.y = pm::neg<Q>(P.p.y);
            Bytes u, c;
            ser_g1_uncompressed<C>(P, u);
            ser_g1<C>(P, c);
            Reader ru(u.data(), u.size()), rc(c.data(), c.size());
            const G1Point<C> pu = deser_g1_uncompressed<C>(ru), pc = deser_g1<C>(rc);
            check(u.size() == (size_t)2 * NB && same<C>(pu, pc) && same<C>(pu, P), curve, "k G in both forms, k = " + std::to_string(k));
            if (!bls) check(((u[flag_at] & 0x80) != 0) == ((c[NB - 1] & 0x80) != 0), curve, "sign bit written as the compressed form writes it");
        }
    }

    // ---- refusals, each with its text
    uint32_t p[NW], p1[NW], ones[NW];
    for (int i = 0; i < NW; ++i) { p[i] = Q::MOD[i]; p1[i] = Q::MOD[i]; ones[i] = 0xFFFFFFFFu; }
    p1[0] += 1;                                        // p is odd: no carry
    const std::string GE = "G1: coordinate >= p", NONCANON = "G1: non-canonical encoding of the point at infinity";
    for (int validate = 0; validate < 2; ++validate) {
        const bool v = validate != 0;
        Bytes r;
        if (bls) {
            r = gen; r[0] |= 0x80;
            check(refusal<C>(r, v) == "G1: not an uncompressed point", curve, "compressed bit");
            r = gen; r[0] |= 0x20;
            check(refusal<C>(r, v) == "G1: not an uncompressed point", curve, "sort bit on a finite point");
            r = inf; r[0] |= 0x20;
            check(refusal<C>(r, v) == "G1: sign bit on the point at infinity", curve, "sort bit on infinity");
            r = inf; r[0] |= 0x80;
            check(refusal<C>(r, v) == "G1: not an uncompressed point", curve, "compressed infinity");
        } else {
            r = inf; r[flag_at] |= 0x80;
            check(refusal<C>(r, v) == "G1: both flag bits set", curve, "both flag bits");
            r = gen; r[flag_at] |= 0xC0;
            check(refusal<C>(r, v) == "G1: both flag bits set", curve, "both flag bits on a coordinate pair");
        }
        r = inf; r[5] |= 0x01;
        check(refusal<C>(r, v) == NONCANON, curve, "stray bit in the x half of infinity");
        r = inf; r[NB + 7] |= 0x10;
        check(refusal<C>(r, v) == NONCANON, curve, "stray bit in the y half of infinity");
        r = inf; r[bls ? 0 : flag_at] |= 0x01;
        check(refusal<C>(r, v) == NONCANON, curve, "stray bit in the flag byte of infinity");
        r = gen; put_coord<C>(r, 0, p);
        check(refusal<C>(r, v) == GE, curve, "x = p");
        r = gen; put_coord<C>(r, 1, p);
        check(refusal<C>(r, v) == GE, curve, "y = p");
        r = gen; put_coord<C>(r, 0, p1);
        check(refusal<C>(r, v) == GE, curve, "x = p + 1");
        r = gen; put_coord<C>(r, 1, p1);
        check(refusal<C>(r, v) == GE, curve, "y = p + 1");
        if (bls) {   // y uses all of its 384 bits: the top three are value, not flags
            r = gen; put_coord<C>(r, 1, ones);
            check(refusal<C>(r, v) == GE, curve, "y = 2^384 - 1");
        } else {     // x uses all of its 256 bits
            r = gen; put_coord<C>(r, 0, ones);
            check(refusal<C>(r, v) == GE, curve, "x = 2^256 - 1");
        }
        // (x, y + 1): off the curve with validation off too
        G1Point<C> off = G;
        off.p.y = pm::add<Q>(off.p.y, pm::Fp<Q>::one());
        r.clear();
        ser_g1_uncompressed<C>(off, r);
        check(refusal<C>(r, v) == "G1: not on the curve", curve, "(x, y + 1)");
    }
    if (bls) {   // a curve point outside G1: the cofactor is ~2^126, so the first x with a square x^3 + 4 is one
        G1Point<C> T;
        T.inf = false;
        pm::Fp<Q> bb;
        for (int i = 0; i < NW; ++i) bb.l[i] = C::B_MONT[i];
        pm::Fp<Q> x = pm::Fp<Q>::one();
        for (;;) {
            x = pm::add<Q>(x, pm::Fp<Q>::one());
            if (fq_sqrt<Q>(pm::add<Q>(pm::mul<Q>(pm::sqr<Q>(x), x), bb), T.p.y)) break;
        }
        T.p.x = x;
        check(!g1_in_subgroup<C>(T), curve, "the probe point is outside G1");
        Bytes r;
        ser_g1_uncompressed<C>(T, r);
        check(refusal<C>(r, true) == "G1: not in the prime-order subgroup", curve, "outside G1, validated");
        check(refusal<C>(r, false).empty(), curve, "outside G1, not validated");
    } else {     // ark's "y > -y" bit set and clear on the same point: both accepted, the same point
        Bytes set = gen, clear = gen;
        set[flag_at] |= 0x80;
        clear[flag_at] &= 0x7F;
        Reader rs(set.data(), set.size()), rc(clear.data(), clear.size());
        check(same<C>(deser_g1_uncompressed<C>(rs), G) && same<C>(deser_g1_uncompressed<C>(rc), G), curve, "sign bit set and clear");
    }
    {   // truncated record
        Bytes r(gen.begin(), gen.end() - 1);
        check(refusal<C>(r, true) == "truncated key", curve, "truncated record");
    }

    // ---- G2: both ways, the sign, infinity, refusals
    const uint32_t five[1] = {5}, seven[1] = {7};
    const typename B::G2 g2 = B::g2_generator(), x2 = B::g2_mul(g2, five, 1), z2 = B::g2_neg(B::g2_mul(g2, seven, 1));
    for (const typename B::G2 &q : {g2, x2, z2}) {
        Bytes u, c;
        ser_g2_uncompressed<C>(q, u);
        ser_g2_c<C>(q, c);
        Reader ru(u.data(), u.size()), rc(c.data(), c.size());
        const typename B::G2 qu = deser_g2_uncompressed<C>(ru), qc = deser_g2_c<C>(rc);
        check(u.size() == (size_t)4 * NB && !qu.inf && qu.x.eq(q.x) && qu.y.eq(q.y) && qc.x.eq(qu.x) && qc.y.eq(qu.y), curve, "G2 in both forms");
        Bytes bad = u;
        bad[bls ? 4 * NB - 1 : 2 * NB] ^= 1;           // the low byte of y.c0
        std::string why;
        try { Reader rb(bad.data(), bad.size()); deser_g2_uncompressed<C>(rb); } catch (const WireError &e) { why = e.what(); }
        check(why == "G2: not on the twist", curve, "G2 off the twist: " + why);
        if (bls) {
            bad = u; bad[0] |= 0x80;
            why.clear();
            try { Reader rb(bad.data(), bad.size()); deser_g2_uncompressed<C>(rb); } catch (const WireError &e) { why = e.what(); }
            check(why == "G2: not an uncompressed point", curve, "G2 compressed bit");
        }
    }
    {
        typename B::G2 o2 = g2;
        o2.inf = true;
        Bytes u;
        ser_g2_uncompressed<C>(o2, u);
        Bytes expect(4 * NB, 0);
        expect[bls ? 0 : 4 * NB - 1] = 0x40;
        Reader ru(u.data(), u.size());
        check(u == expect && deser_g2_uncompressed<C>(ru).inf, curve, "G2 infinity");
        u[NB] = 1;
        std::string why;
        try { Reader rb(u.data(), u.size()); deser_g2_uncompressed<C>(rb); } catch (const WireError &e) { why = e.what(); }
        check(why == "G2: non-canonical encoding of the point at infinity", curve, "G2 stray bit on infinity");
    }

    // ---- the vk: 728 / 504 bytes, and back to the compressed bytes
    VerifyingKeyT<C> vk;
    vk.one_g1 = G; vk.one_g2 = g2; vk.x_g2 = x2; vk.z_g2 = z2;
    vk.n = 8; vk.m0 = 2; vk.sigma = 11;
    vk.omega = pm::Fp<typename C::FrP>::one();
    Bytes vc, vu, back;
    ser_vk_c<C>(vk, vc);
    ser_vk_c<C>(vk, vu, PM_WIRE_UNCOMPRESSED);
    check(vc.size() == vk_c && vu.size() == vk_u, curve, "vk lengths " + std::to_string(vc.size()) + " / " + std::to_string(vu.size()));
    ser_vk_c<C>(read_vk_exact<C>(vu.data(), vu.size(), PM_WIRE_UNCOMPRESSED), back);
    check(back == vc, curve, "vk uncompressed -> compressed");
    back.clear();
    ser_vk_c<C>(read_vk_exact<C>(vc.data(), vc.size()), back, PM_WIRE_UNCOMPRESSED);
    check(back == vu, curve, "vk compressed -> uncompressed");
    for (int wrong = 0; wrong < 2; ++wrong) {          // no format guessing
        bool threw = false;
        try {
            if (wrong) read_vk_exact<C>(vu.data(), vu.size(), PM_WIRE_COMPRESSED);
            else read_vk_exact<C>(vc.data(), vc.size(), PM_WIRE_UNCOMPRESSED);
        } catch (const WireError &) { threw = true; }
        check(threw, curve, "vk of the other form refused");
    }
    bool threw = false;
    try { ser_vk_c<C>(vk, back, 1); } catch (const WireError &) { threw = true; }
    check(threw, curve, "unknown form refused");
    printf("%s: %d failures of %d\n", curve, fails, checks);
}

int main(int argc, char **argv) {
    run<pm::BlsCurve>("bls12_381",
                      "17f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb"
                      "08b3f481e3aaa0f1a09e30ed741d8ae4fcf5e095d5d00af600db18cb2c04b3edd03cc744a2888ae40caa232946c5e7e1",
                      "40" + std::string(190, '0'), 392, 728);
    const int bls_fails = fails;
    fails = checks = 0;
    run<pm::BnCurve>("bn254", "01" + std::string(62, '0') + "02" + std::string(62, '0'), std::string(126, '0') + "40", 280, 504);
    fails += bls_fails;
    // golden keys: compressed -> WireKey -> uncompressed -> WireKey -> compressed is the identity
    typedef pm::BlsCurve C;
    for (int a = 1; a < argc; ++a) {
        std::ifstream f(argv[a]);
        std::string hex;
        f >> hex;
        const Bytes data = unhex(hex);
        try {
            const WireKey<C> k = WireKey<C>::parse(data.data(), data.size());
            const Bytes wide = k.to_bytes(PM_WIRE_UNCOMPRESSED);
            size_t pts = 0;
            for (auto &v : k.vec) pts += v.size();
            const bool len_ok = wide.size() == data.size() + 48 * pts + (728 - 392);
            const WireKey<C> k2 = WireKey<C>::parse(wide.data(), wide.size(), true, PM_WIRE_UNCOMPRESSED);
            const bool id_ok = k2.to_bytes() == data && k2.to_bytes(PM_WIRE_UNCOMPRESSED) == wide;
            bool t1 = false, t2 = false, t3 = false, t4 = false;
            try { WireKey<C>::parse(wide.data(), wide.size(), true, PM_WIRE_COMPRESSED); } catch (const WireError &) { t1 = true; }
            try { WireKey<C>::parse(data.data(), data.size(), true, PM_WIRE_UNCOMPRESSED); } catch (const WireError &) { t2 = true; }
            try { WireKey<C>::parse(wide.data(), wide.size() - 1, true, PM_WIRE_UNCOMPRESSED); } catch (const WireError &) { t3 = true; }
            Bytes more = wide;
            more.push_back(0);
            try { WireKey<C>::parse(more.data(), more.size(), true, PM_WIRE_UNCOMPRESSED); } catch (const WireError &) { t4 = true; }
            if (len_ok && id_ok && t1 && t2 && t3 && t4) printf("wire ok points=%zu bytes=%zu uncompressed=%zu\n", pts, data.size(), wide.size());
            else { fails++; printf("key FAILED len=%d identity=%d refusals=%d%d%d%d: %s\n", len_ok, id_ok, t1, t2, t3, t4, argv[a]); }
        } catch (const std::exception &e) { fails++; printf("parse failed: %s (%s)\n", e.what(), argv[a]); }
    }
    printf("wire uncompressed selftest: %d failures\n", fails);
    return fails ? 1 : 0;
}
