// Batch verification, the per-proof elliptic-curve work (include/polymath_hip.h: pm_verify_batch; DESIGN.md "Batch verification").
//
// For proof i with weight rho_i the host needs
//     U_i = rho_i A_i + (rho_i x2_i) C_i        V_i = rho_i D_i        W_i = (rho_i x1_i) D_i
// and, for the bisection, the sums of these over every aligned power-of-two range of proofs.  verify_term computes one (U, V, W)
// on the reduced-radix registers of fq28.cuh, verify_tree_add one node of the binary sum tree.  Both are PM_HD: the kernels below
// run them one proof / one node coordinate per lane, tests/native/verify_batch_selftest.cpp runs them on the host against the
// dense double-and-add of Polymath::verify.
//
// The points are the prover's, i.e. an attacker's: A = +-C, points at infinity and partial sums that meet or cancel all happen
// when somebody wants them to.  Every addition therefore goes through the fast formulas' own verdict (xyzz28_madd / xyzz28_add
// return false on equal x) into the complete dense formulas (xyzz28_madd_exceptional / xyzz28_add_exceptional); the point at
// infinity is skipped by the caller, as the group law says.  xyzz28_dbl needs Y != 0 on a finite point: both groups have odd
// order, and the decode kernel (validate = 1) has put every point into them.
#pragma once
#include "fq28.cuh"

namespace pm {

// One proof's scalars, canonical (NOT Montgomery) little-endian 32-bit words.  A proof that takes no part (malformed) has all zero.
struct VerifyScalars {
    uint32_t rho[4];   // rho            < 2^128: multiplies A (in U) and D (in V)
    uint32_t rx2[8];   // rho x2 mod r:  multiplies C (in U)
    uint32_t rx1[8];   // rho x1 mod r:  multiplies D (in W)
};

// One leaf or node of the sum tree: three points, XYZZ in STANDARD Montgomery form (what the host's xyzz_to_affine takes).
template <class C>
struct VerifyTerm {
    XYZZ<C> U, V, W;
};

template <class C>
PM_HD XYZZ28<C> xyzz28_identity() {
    typedef typename C::FqRR RR;
    XYZZ28<C> z;
    z.X = z.Y = z.ZZ = z.ZZZ = f28_zero<RR>();
    return z;
}

// k1 P1 + k2 P2 by a joint double-and-add (Straus: one chain of doublings for both scalars).  k1 has n1 <= 8 words, k2 has 8;
// the chain starts at the top word that can hold a set bit.  P1, P2: affine, STANDARD Montgomery form, either may be the point
// at infinity (x = y = 0), and then its scalar is ignored.
template <class C>
PM_HD XYZZ28<C> verify_straus(const Affine<C> &p1_std, const uint32_t *k1, int n1, const Affine<C> &p2_std, const uint32_t *k2, int n2) {
    typedef typename C::FqRR RR;
    typedef F28<RR> F;
    const bool live1 = n1 > 0 && !p1_std.is_inf(), live2 = n2 > 0 && !p2_std.is_inf();
    // the reduced-radix formulas take the INTERNAL radix, on 28-bit limbs: converted and unpacked once per chain
    const Affine<C> p1{fq_std_to_int<C>(p1_std.x), fq_std_to_int<C>(p1_std.y)}, p2{fq_std_to_int<C>(p2_std.x), fq_std_to_int<C>(p2_std.y)};
    const F x1 = f28_unpack<RR>(p1.x.l), y1 = f28_unpack<RR>(p1.y.l), x2 = f28_unpack<RR>(p2.x.l), y2 = f28_unpack<RR>(p2.y.l);
    XYZZ28<C> acc = xyzz28_identity<C>();
    const int top = (n1 > n2 ? n1 : n2) - 1;
#pragma unroll 1
    for (int i = top; i >= 0; --i) {
        const uint32_t w1 = live1 && i < n1 ? k1[i] : 0u, w2 = live2 && i < n2 ? k2[i] : 0u;
#pragma unroll 1
        for (int b = 31; b >= 0; --b) {
            xyzz28_dbl<C>(acc);
            // ONE mixed-addition site for both points (the body is ~5 k instructions): the operand is selected limb by limb
#pragma unroll 1
            for (int s = 0; s < 2; ++s) {
                if (!(((s ? w2 : w1) >> b) & 1u)) continue;
                F qx, qy;
#pragma unroll
                for (int k = 0; k < RR::N; ++k) { qx.l[k] = s ? x2.l[k] : x1.l[k]; qy.l[k] = s ? y2.l[k] : y1.l[k]; }
                if (!xyzz28_madd_limbs<C>(acc, qx, qy, false)) acc = xyzz28_madd_exceptional<C>(acc, s ? p2 : p1, false);   // acc == +-Q
            }
        }
    }
    return acc;
}

// (U, V, W) of one proof.  pts: A, C, D as the decode kernel leaves them (affine, standard Montgomery form, infinity = all-zero).
template <class C>
PM_HD void verify_term(const Affine<C> *pts, const VerifyScalars *sc, VerifyTerm<C> *out) {
    const Affine<C> none = Affine<C>::infinity();
    // U = rho A + rx2 C, V = rho D + 0, W = 0 + rx1 D: three runs of ONE chain body (D is read once per run it takes part in)
#pragma unroll 1
    for (int ph = 0; ph < 3; ++ph) {
        const Affine<C> p1 = ph == 2 ? none : pts[ph == 0 ? 0 : 2], p2 = ph == 1 ? none : pts[ph == 0 ? 1 : 2];
        const XYZZ28<C> r = verify_straus<C>(p1, sc->rho, ph == 2 ? 0 : 4, p2, ph == 0 ? sc->rx2 : sc->rx1, ph == 1 ? 0 : 8);
        (&out->U)[ph] = xyzz28_to_std<C>(r);   // U, V, W are three XYZZ<C> in a row
    }
}

// a + b for one coordinate of a tree node (both in standard Montgomery form, either may be the identity); complete.
template <class C>
PM_HD XYZZ<C> verify_tree_add(const XYZZ<C> &a_std, const XYZZ<C> &b_std) {
    XYZZ28<C> a = xyzz28_from_std<C>(a_std);
    xyzz28_add_full<C>(a, xyzz28_from_std<C>(b_std));
    return xyzz28_to_std<C>(a);
}

// The scalar glue of one proof, for the challenge lanes (challenges.hip) and for the host's threads alike.  sc.rho holds the weight
// on entry; sc.rx2 = rho x2 and sc.rx1 = rho x1 (canonical) are filled in, and g = rho (a(x1) + x2 c(x1)) (Montgomery) comes back.
// A row that is not live -- a(x1) not canonical, a refused point -- has no weight: an all-zero record and g = 0, it never enters a sum.
template <class C>
PM_HD Fp<typename C::FrP> verify_weigh(VerifyScalars &sc, const Fp<typename C::FrP> &x1, const Fp<typename C::FrP> &x2,
                                       const Fp<typename C::FrP> &c_at_x1, const Fp<typename C::FrP> &a_at_x1, bool live) {
    typedef typename C::FrP P;
    typedef Fp<P> Fr;
    Fr rho = Fr::zero();
#pragma unroll
    for (int k = 0; k < 4; ++k) rho.l[k] = sc.rho[k];
    rho = to_mont<P>(rho);
    const Fr rx2 = from_mont<P>(mul<P>(rho, x2)), rx1 = from_mont<P>(mul<P>(rho, x1));
#pragma unroll
    for (int k = 0; k < 8; ++k) { sc.rx2[k] = rx2.l[k]; sc.rx1[k] = rx1.l[k]; }
    Fr g = mul<P>(rho, add<P>(a_at_x1, mul<P>(x2, c_at_x1)));
    if (!live) { sc = VerifyScalars{}; g = Fr::zero(); }
    return g;
}

// The G1 side of a tree node's equation  e(U - g G, [z]_2) e(-V, [x]_2) e(W, [1]_2) == 1:  P = {U + neg_g G, -V, W}, affine, the
// identity as infinity.  neg_g: -g mod r in 8 canonical words.  One lane of k_pairing_check (pairing_batch.hip) or one host check.
template <class C>
PM_HD void verify_node_points(const VerifyTerm<C> &node, const uint32_t *neg_g, const Affine<C> &G, Affine<C> P[3]) {
    const XYZZ<C> lhs = xyzz_add<C>(node.U, xyzz_mul_words<C>(G, neg_g, 8));   // G = O: U itself
    P[0] = xyzz_to_affine<C>(lhs);
    P[1] = xyzz_to_affine<C>(node.V);
    P[1].y = neg<typename C::FqP>(P[1].y);
    P[2] = xyzz_to_affine<C>(node.W);
}

// The tree over `padded` = 2^depth leaves lives in one array of 2 padded - 1 nodes: level l (0 = leaves) holds padded >> l nodes
// from verify_level_offset(padded, l) on; the root is the last node.
PM_HD size_t verify_level_offset(size_t padded, unsigned level) { return 2 * padded - (2 * padded >> level); }

#if defined(__HIPCC__)
// One proof per lane.  status: the decode kernel's three verdicts per proof; a proof with a refused point is a leaf of identities
// (the host gives it no weight either).  Lanes count .. padded - 1 write the padding leaves.
template <class C>
__global__ __launch_bounds__(256, 1) void k_verify_terms(const Affine<C> *pts, const uint8_t *status, const VerifyScalars *sc, size_t count,
                                                        size_t padded, VerifyTerm<C> *leaves) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= padded) return;
    const bool live = i < count && (status[3 * i] | status[3 * i + 1] | status[3 * i + 2]) == 0;
    if (!live) {
        leaves[i].U = leaves[i].V = leaves[i].W = XYZZ<C>::identity();
        return;
    }
    verify_term<C>(pts + 3 * i, sc + i, leaves + i);
}

// One level of the sum tree: lane t adds coordinate t % 3 (U, V, W) of the children 2 j, 2 j + 1 of node j = t / 3.
template <class C>
__global__ __launch_bounds__(256, 1) void k_verify_tree(const VerifyTerm<C> *below, VerifyTerm<C> *level, size_t nodes) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 3 * nodes) return;
    const size_t j = t / 3, c = t % 3;
    const XYZZ<C> *l = &below[2 * j].U + c, *r = &below[2 * j + 1].U + c;   // U, V, W are three XYZZ<C> in a row
    (&level[j].U)[c] = verify_tree_add<C>(*l, *r);
}
#endif

}  // namespace pm
