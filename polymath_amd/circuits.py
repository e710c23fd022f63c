"""Workload generators: the reference's harness circuits as ConstraintSynthesizer-shaped classes
(tests/dummy.rs:20-35, tests/mimc.rs:74-143, benches/bench.rs:38-61) and the synthetic
"random A*B=C gates" R1CS BASELINE.json quotes the headline metric on, and two boolean circuits of this project's
own (RangeCheck, ArxDemo) whose witnesses the device completes from the inputs (PM_ASSIGNMENT_SOLVE)."""
from .polymath import ConstraintSystem, Field, LimbCircuit, R1CS

SPLITMIX_SEED = 0x706F6C796D617468  # "polymath"
_M64 = (1 << 64) - 1


class SplitMix64:
    def __init__(self, seed=SPLITMIX_SEED):
        self.s = seed & _M64

    def next_u64(self):
        self.s = (self.s + 0x9E3779B97F4A7C15) & _M64
        z = self.s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
        return z ^ (z >> 31)

    def fr(self, r):
        nb = r.bit_length()
        while True:
            v = 0
            for i in range(4):
                v |= self.next_u64() << (64 * i)
            v &= (1 << nb) - 1
            if v < r:
                return v


class DummyCircuit:
    """tests/dummy.rs:20-35: witnesses a, b; public c = a*b; a * b = c."""

    def __init__(self, a, b):
        self.a, self.b = a, b

    def generate_constraints(self, cs):
        a = cs.new_witness_variable(self.a)
        b = cs.new_witness_variable(self.b)
        c = cs.new_input_variable(self.a * self.b)
        cs.enforce_constraint([(1, a)], [(1, b)], [(1, c)])


class BenchCircuit:
    """benches/bench.rs:38-61."""

    def __init__(self, a, b, num_variables, num_constraints):
        self.a, self.b, self.nv, self.nc = a, b, num_variables, num_constraints

    def generate_constraints(self, cs):
        a = cs.new_witness_variable(self.a)
        b = cs.new_witness_variable(self.b)
        c = cs.new_input_variable(self.a * self.b)
        for _ in range(self.nv - 3):
            cs.new_witness_variable(self.a)
        for _ in range(self.nc - 1):
            cs.enforce_constraint([(1, a)], [(1, b)], [(1, c)])
        cs.enforce_constraint([], [], [])


class MiMCDemo:
    """tests/mimc.rs:66-143 (LongsightF322p3 when len(constants) == 322)."""

    def __init__(self, xl, xr, constants):
        self.xl, self.xr, self.constants = xl, xr, constants

    def generate_constraints(self, cs):
        r = cs.r
        xl_v, xr_v = self.xl % r, self.xr % r
        xl, xr = cs.new_witness_variable(xl_v), cs.new_witness_variable(xr_v)
        n = len(self.constants)
        for i, ci in enumerate(self.constants):
            tmp_v = pow(xl_v + ci, 2, r)
            tmp = cs.new_witness_variable(tmp_v)
            lc = [(1, xl), (ci, ConstraintSystem.ONE)]
            cs.enforce_constraint(lc, lc, [(1, tmp)])
            new_v = ((xl_v + ci) * tmp_v + xr_v) % r
            new_xl = cs.new_input_variable(new_v) if i == n - 1 else cs.new_witness_variable(new_v)
            cs.enforce_constraint([(1, tmp)], lc, [(1, new_xl), (r - 1, xr)])
            xr, xr_v = xl, xl_v
            xl, xl_v = new_xl, new_v


def mimc_native(r, xl, xr, constants):
    for ci in constants:
        xl, xr = (pow(xl + ci, 3, r) + xr) % r, xl
    return xl


def _new_boolean(cs, bit):
    """Boolean::new_witness: the variable, then its booleanity row  b * (1 - b) = 0"""
    b = cs.new_witness_variable(bit)
    cs.enforce_constraint([(1, b)], [(1, ConstraintSystem.ONE), (-1, b)], [])
    return b


def _new_bits(cs, value, count):
    """`count` boolean witnesses, least significant first, with their booleanity rows (before the row that will fix them)"""
    return [_new_boolean(cs, (value >> i) & 1) for i in range(count)]


def _weighted(bits):
    return [(1 << i, b) for i, b in enumerate(bits)]


class _Partial:
    """What the boolean generators share: which witness values the caller chooses; everything else is for the device
    (PM_ASSIGNMENT_SOLVE) -- every bit is fixed by a decomposition row or by an ordinary row, every sum by an ordinary row."""

    def _given(self, cs, value):
        self._chosen.append(len(cs.witness))
        return cs.new_witness_variable(value)

    def partial(self, r):
        """-> (instance, witness) as ints with None where the device solves (Polymath.partial_limbs takes them)"""
        cs = ConstraintSystem(r)
        self.generate_constraints(cs)
        witness = [None] * len(cs.witness)
        for j in self._chosen:
            witness[j] = cs.witness[j]
        return [1] + [None] * (len(cs.instance) - 1), witness


class RangeCheck(_Partial):
    """N independent range checks v < 2^bits: per value the witness v, `bits` boolean witnesses with their booleanity rows, and
    the row  v * 1 = sum 2^i b_i  (bits in C).  One dependency level of N decompositions.  Witness layout: v, b_0 .. b_{bits-1} per
    value; no public input.  Given v only, the device computes the bits; v >= 2^bits has no assignment (generate_constraints keeps
    the low bits, the solver reports the row as stuck)."""

    def __init__(self, values, bits):
        self.values, self.bits = list(values), bits

    def generate_constraints(self, cs):
        self._chosen = []
        for value in self.values:
            v = self._given(cs, value)
            bits = _new_bits(cs, value, self.bits)
            cs.enforce_constraint([(1, v)], [(1, ConstraintSystem.ONE)], _weighted(bits))

    def native(self):
        """the witness as the rows define it: per value v and its bits"""
        out = []
        for value in self.values:
            out += [value] + [(value >> i) & 1 for i in range(self.bits)]
        return out


class ArxDemo(_Partial):
    """An add-rotate-xor toy permutation on two `width`-bit words, the shape of SHA-256's and ChaCha's inner steps.  Per round:
        a, b           decomposed into `width` bits each                                  (sum 2^i a_i) * 1 = a     bits in A
        s = a + b      decomposed into width + 1 bits                                     (a + b) * 1 = sum 2^i s_i bits in C
        x_i            = s_i xor b_{(i + rot) mod width},  i < width                      (2 s_i) * b_j = s_i + b_j - x_i
        a' = sum 2^i x_i,  b' = sum_{i < width} 2^i s_i                                   two ordinary rows
    Every bit is a Boolean::new_witness (its booleanity row comes before the row that fixes it, as arkworks emits them); the last a'
    is the public input.  The caller chooses a and b; arx_native gives the output."""

    def __init__(self, a, b, width, rounds, rot):
        assert 0 <= a < 1 << width and 0 <= b < 1 << width and 0 < rot < width and rounds >= 1
        self.a, self.b, self.width, self.rounds, self.rot = a, b, width, rounds, rot

    def generate_constraints(self, cs):
        self._chosen = []
        one, width, mask = ConstraintSystem.ONE, self.width, (1 << self.width) - 1
        a_v, b_v = self.a, self.b
        a, b = self._given(cs, a_v), self._given(cs, b_v)
        for rnd in range(self.rounds):
            a_bits = _new_bits(cs, a_v, width)
            cs.enforce_constraint(_weighted(a_bits), [(1, one)], [(1, a)])
            b_bits = _new_bits(cs, b_v, width)
            cs.enforce_constraint(_weighted(b_bits), [(1, one)], [(1, b)])
            s_v = a_v + b_v
            s_bits = _new_bits(cs, s_v, width + 1)
            cs.enforce_constraint([(1, a), (1, b)], [(1, one)], _weighted(s_bits))
            x_v = (s_v & mask) ^ _rotr(b_v, self.rot, width)
            x_bits = []
            for i in range(width):
                x = _new_boolean(cs, (x_v >> i) & 1)
                bj = b_bits[(i + self.rot) % width]
                cs.enforce_constraint([(2, s_bits[i])], [(1, bj)], [(1, s_bits[i]), (1, bj), (-1, x)])
                x_bits.append(x)
            a_v, b_v = x_v, s_v & mask
            a = cs.new_input_variable(a_v) if rnd == self.rounds - 1 else cs.new_witness_variable(a_v)
            cs.enforce_constraint(_weighted(x_bits), [(1, one)], [(1, a)])
            b = cs.new_witness_variable(b_v)
            cs.enforce_constraint(_weighted(s_bits[:width]), [(1, one)], [(1, b)])


def _rotr(v, rot, width):
    return ((v >> rot) | (v << (width - rot))) & ((1 << width) - 1)


def arx_native(a, b, width, rounds, rot):
    """ArxDemo's public output on plain integers"""
    mask = (1 << width) - 1
    for _ in range(rounds):
        s = a + b
        a, b = (s & mask) ^ _rotr(b, rot, width), s & mask
    return a


def synthetic_r1cs(r, nr, seed=SPLITMIX_SEED):
    """m0 = 2; gate i: A_i = {(alpha_i, p_i)}, B_i = {(beta_i, q_i)}, C_i = {(1, t_i)},
    t_i = (alpha_i z_p)(beta_i z_q); p, q uniform over already-defined variables; the last gate's
    output is the public input.  Draw order: w0, w1, then per gate alpha, beta, p, q."""
    g = SplitMix64(seed)
    m0 = 2
    wit = [g.fr(r), g.fr(r)]
    cols, vals = [0, m0, m0 + 1], [1, wit[0], wit[1]]
    A, B, C = [], [], []
    pub = None
    for i in range(nr):
        alpha, beta = g.fr(r), g.fr(r)
        pi, qi = g.next_u64() % len(cols), g.next_u64() % len(cols)
        t = (alpha * vals[pi] % r) * (beta * vals[qi] % r) % r
        if i == nr - 1:
            col, pub = 1, t
        else:
            col = m0 + len(wit)
            wit.append(t)
            cols.append(col)
            vals.append(t)
        A.append([(alpha, cols[pi])])
        B.append([(beta, cols[qi])])
        C.append([(1, col)])
    return R1CS(m0, len(wit), A, B, C), [1, pub], wit


def synthetic_r1cs_native(curve, nr, seed=SPLITMIX_SEED):
    """The same circuit and assignment as synthetic_r1cs, generated by the library (pm_synth_r1cs) straight into
    limb arrays: seconds instead of minutes at 2^24 gates.  -> LimbCircuit."""
    from . import api
    csrs, inst, wit = api.synth_r1cs(curve, nr, seed)
    return LimbCircuit(Field(curve), 2, nr + 1, nr, csrs, inst, wit)
