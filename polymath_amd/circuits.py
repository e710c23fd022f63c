"""Workload generators: the reference's harness circuits as ConstraintSynthesizer-shaped classes
(tests/dummy.rs:20-35, tests/mimc.rs:74-143, benches/bench.rs:38-61) and the synthetic
"random A*B=C gates" R1CS BASELINE.json quotes the headline metric on, and two boolean circuits of this project's
own (RangeCheck, ArxDemo) and two that branch on equality (MatchCount, EqChain: is-zero pairs in arkworks' and in circom's form) whose
witnesses the device completes from the inputs (PM_ASSIGNMENT_SOLVE), and two that divide integers (DivRem,
ModChain: Euclidean division rows, whose quotients partial() marks QUOTIENT), and two that read a table at a signal (Decoder,
TableWalk: circomlib's one-hot decoder, whose outputs partial() marks INDICATOR), and two that take square roots (SquareRoots,
EdwardsDecompress: point decompression on Jubjub / Baby Jubjub, whose roots partial() marks SQRT), and three whose rows are square linear systems in their unknowns (LimbProduct, ProductChain: non-native
multiplication, whose product limbs are pinned at 2l - 1 points; LinearBlocks: random systems), which the solver takes as linear blocks, and two that multiply modulo a foreign prime (LimbModMul, ModMulChain: the product's block, then the
quotient and remainder limbs of the reduction, which no row determines: hints() is the long division the key declares for them), and two that divide modulo a foreign modulus (LimbModDiv: a non-native
modular division or inverse; EcAddChain: affine point additions, whose slopes are such divisions: hints() declares a modular hint for each
and a long division for every reduction); Reordered emits any of them with its rows in another
order, which the solver's any-order planner accepts."""
from .polymath import INDICATOR, QUOTIENT, SQRT, ConstraintSystem, Field, LimbCircuit, R1CS, small_sqrt

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


def _lc_value(cs, lc):
    value = {"one": lambda i: 1, "inst": lambda i: cs.instance[i], "wit": lambda i: cs.witness[i]}
    return sum(coef * value[kind](idx) for coef, (kind, idx) in lc) % cs.r


def _merged(lc):
    """the linear combination with one entry per variable (the matrices keep the FIRST entry of a column that a row names twice)"""
    total = {}
    for coef, var in lc:
        total[var] = total.get(var, 0) + coef
    return [(coef, var) for var, coef in total.items()]


def _new_is_zero(cs, lc, form, free=0):
    """The is-zero / inverse-or-zero pair on the linear combination `lc` (value d): two fresh witnesses, the flag first and then the
    multiplier m, and two rows, the opener and the closer of DESIGN.md §4.10.
        "ark"     (is_neq of arkworks' FpVar): the flag is neq = [d != 0], a Boolean::new_witness with its booleanity row first;
                  lc * m = neq ;  lc * (1 - neq) = 0
        "circom"  (circomlib's IsZero): the flag is out = [d == 0];
                  (-lc) * m = out - 1 ;  lc * out = 0
    m = 1 / d where d != 0; where d == 0 every m satisfies both rows and `free` is written: 0 is what the device computes (circom's
    convention, and what 0^(r-2) gives), 1 is what arkworks' witness generation writes.
    -> (eq, flag, m): eq = the linear combination that is [d == 0], the two variables."""
    one, r = ConstraintSystem.ONE, cs.r
    d = _lc_value(cs, lc)
    m_v = pow(d, r - 2, r) if d else free
    if form == "ark":
        flag = _new_boolean(cs, int(d != 0))
        m = cs.new_witness_variable(m_v)
        cs.enforce_constraint(lc, [(1, m)], [(1, flag)])
        cs.enforce_constraint(lc, [(1, one), (-1, flag)], [])
        return [(1, one), (-1, flag)], flag, m
    if form == "circom":
        flag = cs.new_witness_variable(int(d == 0))
        m = cs.new_witness_variable(m_v)
        cs.enforce_constraint([(-coef, v) for coef, v in lc], [(1, m)], [(1, flag), (-1, one)])
        cs.enforce_constraint(lc, [(1, flag)], [])
        return [(1, flag)], flag, m
    raise ValueError("form is 'ark' or 'circom'")


class _PartialPairs(_Partial):
    """_Partial for circuits with is-zero pairs: partial(r, multipliers=True) gives the multipliers as well (the value generate_constraints
    wrote: 1 / d, or `free` where d == 0), so that only the flags are unknown and every opener is an ordinary kind-C step -- the way
    to get a free multiplier other than the device's 0."""

    def _pair(self, cs, lc):
        eq, _, m = _new_is_zero(cs, lc, self.form, self.free)
        self._multipliers.append(m[1])
        return eq

    def partial(self, r, multipliers=False):
        instance, witness = super().partial(r)
        if multipliers:
            cs = ConstraintSystem(r)
            self.generate_constraints(cs)
            for j in self._multipliers:
                witness[j] = cs.witness[j]
        return instance, witness

    def native(self, r):
        """-> (instance, witness) as the rows define them, on Python integers"""
        cs = ConstraintSystem(r)
        self.generate_constraints(cs)
        return list(cs.instance), list(cs.witness)


class MatchCount(_PartialPairs):
    """How many of `values` equal `key`: per value one is-zero pair on v_i - key, then  (sum e_i) * 1 = count  with e_i = [v_i == key]
    and count the public input.  ONE dependency level of len(values) pairs, then one ordinary step.  Witness layout: key, then per
    value v_i, its flag, its multiplier.  The caller chooses key and the values."""

    def __init__(self, values, key, form, free=0):
        self.values, self.key, self.form, self.free = list(values), key, form, free

    def generate_constraints(self, cs):
        self._chosen, self._multipliers = [], []
        one = ConstraintSystem.ONE
        key = self._given(cs, self.key)
        total = []
        for value in self.values:
            v = self._given(cs, value)
            total += self._pair(cs, [(1, v), (-1, key)])
        count = cs.new_input_variable(sum(int((v - self.key) % cs.r == 0) for v in self.values))
        cs.enforce_constraint(_merged(total), [(1, one)], [(1, count)])


class EqChain(_PartialPairs):
    """A recurrence that branches on equality:  e_i = [s_i == t_i],  s_{i+1} = s_i + 1 + e_i t_i,  s_0 = x.  Per step the witness
    t_i, one is-zero pair on s_i - t_i and the row  e_i * t_i = s_{i+1} - s_i - 1 ; step i's tested value depends on step i - 1's
    flag, so the dependency structure is len(targets) pairs deep and one wide.  With bits > 0 every new state is also range-checked:
    `bits` boolean witnesses and  s_{i+1} * 1 = sum 2^j b_j  (the states must stay below 2^bits).  The last state is the public input.
    The caller chooses x and the targets; eq_chain_targets makes targets that hit and miss where wanted."""

    def __init__(self, x, targets, form, free=0, bits=0):
        self.x, self.targets, self.form, self.free, self.bits = x, list(targets), form, free, bits

    def generate_constraints(self, cs):
        self._chosen, self._multipliers = [], []
        one, r = ConstraintSystem.ONE, cs.r
        s_v = self.x % r
        s = self._given(cs, s_v)
        for i, t_v in enumerate(self.targets):
            t = self._given(cs, t_v)
            eq = self._pair(cs, [(1, s), (-1, t)])
            next_v = (s_v + 1 + (t_v if (s_v - t_v) % r == 0 else 0)) % r
            nxt = cs.new_input_variable(next_v) if i == len(self.targets) - 1 else cs.new_witness_variable(next_v)
            cs.enforce_constraint(eq, [(1, t)], [(1, nxt), (-1, s), (-1, one)])
            if self.bits:
                assert next_v < 1 << self.bits
                cs.enforce_constraint([(1, nxt)], [(1, one)], _weighted(_new_bits(cs, next_v, self.bits)))
            s, s_v = nxt, next_v


def eq_chain_targets(x, hits, r, miss=5):
    """targets for EqChain(x, ...) such that step i finds equality exactly where hits[i]: the state itself, or the state + miss"""
    targets, s = [], x % r
    for hit in hits:
        t = s if hit else (s + miss) % r
        targets.append(t)
        s = (s + 1 + (t if hit else 0)) % r
    return targets


class _PartialDivisions(_Partial):
    """_Partial for circuits with Euclidean division rows  q * b = a - rem  (circom's q <-- a \\ b; rem <-- a % b; q*b + rem === a):
    partial() marks every quotient QUOTIENT -- the explicit "this unknown is a quotient" that the solver asks for, since the row has
    the shape of an is-zero opener -- and leaves the remainders, and the bits of the range checks, None."""

    def _division(self, cs, a_lc, a_v, b, b_v, bits, last_rem=None):
        """witnesses q, rem (or the variable last_rem(rem_v) makes) and, with bits > 0, the boolean witnesses of three range checks
        -- booleanity rows first -- then the division row and  rem * 1 = sum 2^i .. ;  (b - 1 - rem) * 1 = sum 2^i .. ;
        q * 1 = sum 2^i ..  , which make the Euclidean pair the row's only solution.  b_v == 0 has no solution: zeros are written
        (the device reports the row as stuck).  -> (q, rem, q_v, rem_v)"""
        one = ConstraintSystem.ONE
        q_v, rem_v = divmod(a_v, b_v) if b_v else (0, 0)
        self._quotients.append(len(cs.witness))
        q = cs.new_witness_variable(q_v)
        rem = last_rem(rem_v) if last_rem else cs.new_witness_variable(rem_v)
        checks = [([(1, rem)], rem_v), ([(1, b), (-1, one), (-1, rem)], (b_v - 1 - rem_v) % cs.r), ([(1, q)], q_v)] if bits else []
        checks = [(lc, _new_bits(cs, v, bits)) for lc, v in checks]
        cs.enforce_constraint([(1, q)], [(1, b)], a_lc + [(-1, rem)])
        for lc, bit_vars in checks:
            cs.enforce_constraint(lc, [(1, one)], _weighted(bit_vars))
        return q, rem, q_v, rem_v

    def partial(self, r):
        instance, witness = super().partial(r)
        for j in self._quotients:
            witness[j] = QUOTIENT
        return instance, witness

    def native(self, r):
        """-> (instance, witness) as the rows define them, on Python integers"""
        cs = ConstraintSystem(r)
        self.generate_constraints(cs)
        return list(cs.instance), list(cs.witness)


class DivRem(_PartialDivisions):
    """N independent Euclidean divisions of `bits`-bit operands: per pair (a, b) the given witnesses a and b, the witnesses q and rem,
    3 x bits boolean witnesses with their booleanity rows, the division row  q * b = a - rem  and the three range checks of
    _division.  The public input is sum (q_i + rem_i).  ONE dependency level of N divisions, then one of 3 N decompositions, then
    the sum.  The caller chooses the pairs; b = 0 has no assignment."""

    def __init__(self, pairs, bits):
        self.pairs, self.bits = [tuple(p) for p in pairs], bits

    def generate_constraints(self, cs):
        self._chosen, self._quotients = [], []
        total, total_v = [], 0
        for a_v, b_v in self.pairs:
            assert 0 <= a_v < 1 << self.bits and 0 <= b_v < 1 << self.bits
            a, b = self._given(cs, a_v), self._given(cs, b_v)
            q, rem, q_v, rem_v = self._division(cs, [(1, a)], a_v, b, b_v, self.bits)
            total += [(1, q), (1, rem)]
            total_v += q_v + rem_v
        out = cs.new_input_variable(total_v % cs.r)
        cs.enforce_constraint(total, [(1, ConstraintSystem.ONE)], [(1, out)])

    def native(self, r):
        """-> (instance, witness) on Python integers, without generating a row: per pair a, b, q, rem, then the bits of rem, of
        b - 1 - rem and of q, least significant first (what generate_constraints writes)"""
        witness, total = [], 0
        for a, b in self.pairs:
            q, rem = divmod(a, b) if b else (0, 0)
            witness += [a, b, q, rem]
            for v in (rem, (b - 1 - rem) % r, q):
                witness += [(v >> i) & 1 for i in range(self.bits)]
            total += q + rem
        return [1, total % r], witness


class ModChain(_PartialDivisions):
    """A linear congruential recurrence  s_{i+1} = (g s_i + c) mod m  over `steps` steps: the given witnesses s_0, g, c and m, per step
    the product  g * s_i = p_i  and the division row  q_i * m = p_i + c - s_{i+1} ; s_steps is the public input.  Two narrow
    dependency levels per step, so the whole circuit is one run of the solver's chain kernel.  g s_i + c must stay below r (the
    operands are small integers).  With bits > 0 every step carries the three range checks of _division."""

    def __init__(self, s0, g, c, m, steps, bits=0):
        assert steps >= 1
        self.s0, self.g, self.c, self.m, self.steps, self.bits = s0, g, c, m, steps, bits

    def generate_constraints(self, cs):
        self._chosen, self._quotients = [], []
        one = ConstraintSystem.ONE
        s_v = self.s0
        s, g, c, m = (self._given(cs, v) for v in (self.s0, self.g, self.c, self.m))
        for i in range(self.steps):
            p_v = self.g * s_v
            assert p_v + self.c < cs.r
            p = cs.new_witness_variable(p_v)
            cs.enforce_constraint([(1, g)], [(1, s)], [(1, p)])
            last = cs.new_input_variable if i == self.steps - 1 else None
            _, s, _, s_v = self._division(cs, [(1, p), (1, c)], p_v + self.c, m, self.m, self.bits, last_rem=last)


def mod_chain_native(s0, g, c, m, steps):
    """ModChain's public output on plain integers"""
    for _ in range(steps):
        s0 = (g * s0 + c) % m
    return s0


class _PartialIndicators(_Partial):
    """_Partial for circuits with one-hot decoders (circomlib's Decoder:  out[i] <-- (inp == i) ? 1 : 0;  out[i] * (inp - i) === 0):
    partial() marks every out_i INDICATOR -- the explicit "this unknown is the indicator of its guard row" that the solver asks for,
    since the guard does not determine the value where inp == i -- and leaves the sums None."""

    def _decoder(self, cs, inp, inp_v, width):
        """`width` witnesses out_i = [inp == i], each with its guard row  out_i * (inp - i) = 0  (for i = 0 the guard's known side is
        inp alone).  -> (outs, hit): the variables, and 1 where the index is in range, else 0"""
        one, outs = ConstraintSystem.ONE, []
        for i in range(width):
            self._indicators.append(len(cs.witness))
            out = cs.new_witness_variable(int(inp_v == i))
            cs.enforce_constraint([(1, out)], [(1, inp)] + ([(-i, one)] if i else []), [])
            outs.append(out)
        return outs, int(0 <= inp_v < width)

    def partial(self, r):
        instance, witness = super().partial(r)
        for j in self._indicators:
            witness[j] = INDICATOR
        return instance, witness


class Decoder(_PartialIndicators):
    """circomlib's Decoder(width) on the given witness inp: the witnesses out_0 .. out_{width-1} with their guard rows
    out_i * (inp - i) = 0, the sum row  (sum out_i) * 1 = success  with success the public input, and  success * (success - 1) = 0.
    ONE dependency level of `width` indicator rows, then one ordinary step.  Witness layout: inp, then the out_i.  An index out of
    range (width <= inp < r) gives all zeros and success = 0."""

    def __init__(self, width, index):
        assert width >= 1
        self.width, self.index = width, index

    def generate_constraints(self, cs):
        self._chosen, self._indicators = [], []
        one = ConstraintSystem.ONE
        inp_v = self.index % cs.r
        inp = self._given(cs, inp_v)
        outs, hit = self._decoder(cs, inp, inp_v, self.width)
        success = cs.new_input_variable(hit)
        cs.enforce_constraint([(1, out) for out in outs], [(1, one)], [(1, success)])
        cs.enforce_constraint([(1, success)], [(1, success), (-1, one)], [])

    def native(self, r):
        """-> (instance, witness) on Python integers, without generating a row: inp, then out_i = [inp == i]"""
        inp = self.index % r
        return [1, int(inp < self.width)], [inp] + [int(inp == i) for i in range(self.width)]


class TableWalk(_PartialIndicators):
    """Pointer chasing through a table:  idx_{t+1} = table[idx_t],  idx_0 = start, over `steps` steps -- how a circom circuit reads
    RAM, a selector or a jump table at a signal.  Per step one decoder on idx_t (the out_i with their guard rows, the witness
    success_t with  (sum out_i) * 1 = success_t  and  success_t * (success_t - 1) = 0), then
        signals=True    the table entries are given witnesses (allocated once, after idx_0): one product row  out_i * table_i = p_i
                        per entry and the sum  (sum p_i) * 1 = idx_{t+1}
        signals=False   the table entries are constants of the circuit: the one linear row  (sum table_i out_i) * 1 = idx_{t+1}
    The last index is the public input.  An index out of range reads 0.  Indicator levels alternate with ordinary ones (three levels
    per step with signals, two with constants), `len(table)` wide; the batch is the parallel dimension.  The caller chooses start and,
    with signals, the table."""

    def __init__(self, table, start, steps, signals=True):
        assert steps >= 1 and len(table) >= 1
        self.table, self.start, self.steps, self.signals = list(table), start, steps, signals

    def generate_constraints(self, cs):
        self._chosen, self._indicators = [], []
        one, r, width = ConstraintSystem.ONE, cs.r, len(self.table)
        idx_v = self.start % r
        idx = self._given(cs, idx_v)
        entries = [self._given(cs, v) for v in self.table] if self.signals else None
        for t in range(self.steps):
            outs, hit = self._decoder(cs, idx, idx_v, width)
            success = cs.new_witness_variable(hit)
            cs.enforce_constraint([(1, out) for out in outs], [(1, one)], [(1, success)])
            cs.enforce_constraint([(1, success)], [(1, success), (-1, one)], [])
            next_v = self.table[idx_v] % r if hit else 0
            if self.signals:
                products = []
                for i, out in enumerate(outs):
                    products.append(cs.new_witness_variable(self.table[i] if idx_v == i else 0))
                    cs.enforce_constraint([(1, out)], [(1, entries[i])], [(1, products[i])])
                total = [(1, p) for p in products]
            else:
                total = [(v % r, out) for v, out in zip(self.table, outs) if v % r]
            nxt = cs.new_input_variable(next_v) if t == self.steps - 1 else cs.new_witness_variable(next_v)
            cs.enforce_constraint(total, [(1, one)], [(1, nxt)])
            idx, idx_v = nxt, next_v

    def native(self, r):
        """-> (instance, witness) as the rows define them, on Python integers"""
        cs = ConstraintSystem(r)
        self.generate_constraints(cs)
        return list(cs.instance), list(cs.witness)


def table_walk_native(table, start, steps, r):
    """TableWalk's public output on plain integers"""
    idx = start % r
    for _ in range(steps):
        idx = table[idx] % r if idx < len(table) else 0
    return idx


class _PartialRoots(_Partial):
    """_Partial for circuits with square-root rows  u * u = c  (circom's  x <-- sqrt(c); x*x === c): partial() marks every root SQRT --
    the explicit "this unknown is the smaller square root of its row" that the solver asks for, since -u satisfies the row too."""

    def _root(self, cs, c, c_v):
        """the witness u = the smaller root of c_v (0 where c_v is a non-residue: the row has no solution then and the device reports
        it as stuck) with its row  u * u = c.  -> (u, u_v)"""
        u_v = small_sqrt(cs.r, c_v) or 0
        self._roots.append(len(cs.witness))
        u = cs.new_witness_variable(u_v)
        cs.enforce_constraint([(1, u)], [(1, u)], [(1, c)])
        return u, u_v

    def partial(self, r):
        instance, witness = super().partial(r)
        for j in self._roots:
            witness[j] = SQRT
        return instance, witness


class SquareRoots(_PartialRoots):
    """N independent square roots: per value the given witness c_i, the witness u_i and the row  u_i * u_i = c_i ; the public input
    is sum u_i.  ONE dependency level of N square-root rows, then one ordinary step.  Witness layout: c_i, u_i per value.  The caller
    chooses the c_i; a non-residue has no assignment."""

    def __init__(self, values):
        self.values = list(values)

    def generate_constraints(self, cs):
        self._chosen, self._roots = [], []
        total, total_v = [], 0
        for value in self.values:
            c = self._given(cs, value % cs.r)
            u, u_v = self._root(cs, c, value % cs.r)
            total.append((1, u))
            total_v += u_v
        out = cs.new_input_variable(total_v % cs.r)
        cs.enforce_constraint(total, [(1, ConstraintSystem.ONE)], [(1, out)])

    def native(self, r):
        """-> (instance, witness) on Python integers, without generating a row: c_i and its smaller root per value"""
        witness, total = [], 0
        for value in self.values:
            u = small_sqrt(r, value % r) or 0
            witness += [value % r, u]
            total += u
        return [1, total % r], witness


# the twisted Edwards curves  a x^2 + y^2 = 1 + d x^2 y^2  over the two scalar fields: Jubjub over BLS12-381's, Baby Jubjub over BN254's
EDWARDS = {
    0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001: ("jubjub", -1, 0x2A9318E74BFA2B48F5FD9207E6BD7FD4292D7F6D37579D2601065FD6D6343EB1),
    0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001: ("baby_jubjub", 168700, 168696),
}


class EdwardsDecompress(_PartialRoots):
    """Point decompression on the twisted Edwards curve of the field (EDWARDS: Jubjub on BLS12-381, Baby Jubjub on BN254), the shape of
    circomlib's Bits2Point_Strict and of arkworks' decompression gadget.  Per point, from the given witnesses y and sign:
        y * y = y2
        (a - d y2) * u = 1 - y2                   an ordinary dividing step: u = x^2
        x0 * x0 = u                               the square-root row; x0 is marked SQRT
        sign * (1 - sign) = 0                     a check row: sign is given
        x0 * (1 - 2 sign) = x                     the root with the wanted sign
        x0 * 1 = sum 2^i b_i                      bitlength(r) - 1 boolean witnesses, booleanity rows first: the small root always
                                                  fits, so the row never sticks
    and  (sum x) * 1 = out  with out the public input.  The caller chooses the y (edwards_ys draws values for which u is a residue;
    another y has no assignment) and the signs."""

    def __init__(self, ys, signs):
        assert len(ys) == len(signs) and len(ys) >= 1 and all(sg in (0, 1) for sg in signs)
        self.ys, self.signs = list(ys), list(signs)

    def generate_constraints(self, cs):
        self._chosen, self._roots = [], []
        one, r = ConstraintSystem.ONE, cs.r
        _, a, d = EDWARDS[r]
        nbits = r.bit_length() - 1
        total, total_v = [], 0
        for y_v, sign_v in zip(self.ys, self.signs):
            y_v %= r
            y, sign = self._given(cs, y_v), self._given(cs, sign_v)
            y2_v = y_v * y_v % r
            y2 = cs.new_witness_variable(y2_v)
            cs.enforce_constraint([(1, y)], [(1, y)], [(1, y2)])
            den_v = (a - d * y2_v) % r
            u_v = (1 - y2_v) * pow(den_v, r - 2, r) % r
            u = cs.new_witness_variable(u_v)
            cs.enforce_constraint([(a, one), (-d, y2)], [(1, u)], [(1, one), (-1, y2)])
            x0, x0_v = self._root(cs, u, u_v)
            cs.enforce_constraint([(1, sign)], [(1, one), (-1, sign)], [])
            x_v = (r - x0_v) % r if sign_v else x0_v
            x = cs.new_witness_variable(x_v)
            cs.enforce_constraint([(1, x0)], [(1, one), (-2, sign)], [(1, x)])
            cs.enforce_constraint([(1, x0)], [(1, one)], _weighted(_new_bits(cs, x0_v, nbits)))
            total.append((1, x))
            total_v += x_v
        out = cs.new_input_variable(total_v % r)
        cs.enforce_constraint(total, [(1, one)], [(1, out)])

    def native(self, r):
        """-> (instance, witness) on Python integers, without generating a row: per point y, sign, y2, u, x0, x and the bits of x0,
        least significant first (what generate_constraints writes)"""
        _, a, d = EDWARDS[r]
        witness, total = [], 0
        for y, sign in zip(self.ys, self.signs):
            y %= r
            y2 = y * y % r
            u = (1 - y2) * pow((a - d * y2) % r, r - 2, r) % r
            x0 = small_sqrt(r, u) or 0
            x = (r - x0) % r if sign else x0
            witness += [y, sign, y2, u, x0, x] + [(x0 >> i) & 1 for i in range(r.bit_length() - 1)]
            total += x
        return [1, total % r], witness


def edwards_ys(r, count, seed=SPLITMIX_SEED):
    """`count` values y that are the ordinate of a point of the field's Edwards curve (EDWARDS): drawn from SplitMix64(seed), kept
    where a - d y^2 != 0 and (1 - y^2) / (a - d y^2) is a square"""
    _, a, d = EDWARDS[r]
    g, ys = SplitMix64(seed), []
    while len(ys) < count:
        y = g.fr(r)
        den = (a - d * y * y) % r
        if den and small_sqrt(r, (1 - y * y) * pow(den, r - 2, r) % r) is not None:
            ys.append(y)
    return ys


def limb_product(a, b, r):
    """the 2l - 1 limbs of the product of two l-limb numbers without carries, mod r: p_j = sum_{i + i' = j} a_i b_i'"""
    p = [0] * (len(a) + len(b) - 1)
    for i, a_i in enumerate(a):
        for k, b_k in enumerate(b):
            p[i + k] = (p[i + k] + a_i * b_k) % r
    return p


def _product_rows(cs, a, b, p, first):
    """the rows that pin the limbs p of a product: (sum a_i c^i) (sum b_i c^i) = sum p_j c^j  at c = first .. first + len(p) - 1
    (ark-r1cs-std's mul_without_reduce, circom-bigint's BigMultNoCarry); a term whose coefficient is zero (c = 0) is not written"""
    at = lambda limbs, c: [(pow(c, i, cs.r), v) for i, v in enumerate(limbs) if i == 0 or c]
    for c in range(first, first + len(p)):
        cs.enforce_constraint(at(a, c), at(b, c), at(p, c))


class LimbProduct(_Partial):
    """Non-native multiplication: per pair (a, b) of l-limb numbers the given witnesses a_0 .. a_{l-1}, b_0 .. b_{l-1}, the witnesses
    p_0 .. p_{2l-2} of the product's limbs, the 2l - 1 rows of _product_rows at the points first .. first + 2l - 2, and one ordinary row
    (sum p_j) * 1 = s ; the public input is sum s.  Every product row names all 2l - 1 unknowns, so no row order propagates through
    them: the solver takes the rows of a product as ONE linear block, all products sharing one Vandermonde matrix.
    With first = 0 the row at 0 is the ordinary step a_0 b_0 = p_0 and the block has 2l - 2 columns.  The caller chooses the limbs."""

    def __init__(self, products, first=1):
        assert first in (0, 1) and all(len(a) == len(b) and len(a) >= 2 for a, b in products)
        self.products, self.first = [(list(a), list(b)) for a, b in products], first

    def generate_constraints(self, cs):
        self._chosen = []
        one, r = ConstraintSystem.ONE, cs.r
        total, total_v = [], 0
        for a_v, b_v in self.products:
            a = [self._given(cs, v) for v in a_v]
            b = [self._given(cs, v) for v in b_v]
            p_v = limb_product(a_v, b_v, r)
            p = [cs.new_witness_variable(v) for v in p_v]
            _product_rows(cs, a, b, p, self.first)
            s = cs.new_witness_variable(sum(p_v))
            cs.enforce_constraint([(1, v) for v in p], [(1, one)], [(1, s)])
            total.append((1, s))
            total_v += sum(p_v)
        out = cs.new_input_variable(total_v)
        cs.enforce_constraint(total, [(1, one)], [(1, out)])

    def native(self, r):
        """-> (instance, witness) on Python integers, without generating a row: per product the limbs of a, of b, of a b, and their sum"""
        witness, total = [], 0
        for a, b in self.products:
            p = limb_product([v % r for v in a], [v % r for v in b], r)
            witness += [v % r for v in a] + [v % r for v in b] + p + [sum(p) % r]
            total += sum(p)
        return [1, total % r], witness


def limb_products(r, count, limbs, seed=SPLITMIX_SEED):
    """`count` pairs of `limbs`-limb numbers for LimbProduct, every limb a field element drawn from SplitMix64(seed)"""
    g = SplitMix64(seed)
    return [([g.fr(r) for _ in range(limbs)], [g.fr(r) for _ in range(limbs)]) for _ in range(count)]


class ProductChain(_Partial):
    """`steps` non-native products in sequence: x_0 = a and b given (l limbs each); product t is p^t = x_t b (2l - 1 limbs, pinned by
    the rows of _product_rows at the points 1 .. 2l - 1), x_{t+1} = the low l limbs of p^t, and  (sum p^t_j) * 1 = s_t ; the public
    input is sum s_t.  One linear block per dependency level, each followed by the narrow step s_t beside the next block."""

    def __init__(self, a, b, steps):
        assert len(a) == len(b) and len(a) >= 2 and steps >= 1
        self.a, self.b, self.steps = list(a), list(b), steps

    def generate_constraints(self, cs):
        self._chosen = []
        one, r = ConstraintSystem.ONE, cs.r
        x_v, b_v = [v % r for v in self.a], [v % r for v in self.b]
        x = [self._given(cs, v) for v in x_v]
        b = [self._given(cs, v) for v in b_v]
        total, total_v = [], 0
        for _ in range(self.steps):
            p_v = limb_product(x_v, b_v, r)
            p = [cs.new_witness_variable(v) for v in p_v]
            _product_rows(cs, x, b, p, 1)
            s = cs.new_witness_variable(sum(p_v))
            cs.enforce_constraint([(1, v) for v in p], [(1, one)], [(1, s)])
            total.append((1, s))
            total_v += sum(p_v)
            x, x_v = p[:len(x)], p_v[:len(x)]
        out = cs.new_input_variable(total_v)
        cs.enforce_constraint(total, [(1, one)], [(1, out)])

    def native(self, r):
        """-> (instance, witness) on Python integers, without generating a row: a, b, then per product its limbs and their sum"""
        x, b = [v % r for v in self.a], [v % r for v in self.b]
        witness, total = x + b, 0
        for _ in range(self.steps):
            p = limb_product(x, b, r)
            witness += p + [sum(p) % r]
            total += sum(p)
            x = p[:len(x)]
        return [1, total % r], witness


def int_limbs(value, n, count):
    """the `count` n-bit limbs of a non-negative integer, least significant first (the value must fit)"""
    assert 0 <= value < 1 << (n * count)
    return [(value >> (n * i)) & ((1 << n) - 1) for i in range(count)]


def limbs_int(limbs, n):
    """sum limbs_j 2^(n j): the integer of limbs that need not be normalised"""
    return sum(v << (n * j) for j, v in enumerate(limbs))


def modmul_values(a, b, p, n, r):
    """What one non-native modular multiplication witnesses, on Python integers: a, b, p are lists of l limbs of n bits (a and b such
    that no limb of the no-carry product reaches r).  -> (P, q, rem, qp, carries): the 2l - 1 product limbs, the l limbs of
    floor(a b / p) and of a b mod p (Python's divmod), the 2l - 1 limbs of the no-carry product q p mod r, and the 2l - 2 carries of
    P_j - qp_j - rem_j + carry_{j-1} = carry_j 2^n  as field elements (a negative carry is r - |carry|)."""
    l = len(a)
    P = limb_product(a, b, r)
    exact = [sum(a[i] * b[j - i] for i in range(l) if 0 <= j - i < l) for j in range(2 * l - 1)]
    assert P == exact, "a limb of the no-carry product reaches r: D would not be a b"
    q_int, rem_int = divmod(limbs_int(a, n) * limbs_int(b, n), limbs_int(p, n))
    q, rem = int_limbs(q_int, n, l), int_limbs(rem_int, n, l)
    qp_exact = [sum(q[i] * p[j - i] for i in range(l) if 0 <= j - i < l) for j in range(2 * l - 1)]
    carries, carry = [], 0
    for j in range(2 * l - 1):
        total = exact[j] - qp_exact[j] - (rem[j] if j < l else 0) + carry
        assert total % (1 << n) == 0
        carry = total >> n                      # exact: Python's shift of a negative integer floors, and the remainder is zero
        if j < 2 * l - 2:
            carries.append(carry % r)
    assert carry == 0
    return P, q, rem, [v % r for v in qp_exact], carries


class _PartialModMul(_Partial):
    """What LimbModMul and ModMulChain share: one non-native modular multiplication x y mod p on l limbs of n bits, and the hints that
    it declares.  The witnesses, in this order: the 2l - 1 limbs P of the no-carry product (the rows of _product_rows at the points
    1 .. 2l - 1: a linear block), the l limbs of q and the l limbs of rem (HINTED: no row determines them; the hint divides P by p),
    with `decompose` the n booleans of every limb of q and of rem with their booleanity rows and the row  limb * 1 = sum 2^i b_i, the
    2l - 1 limbs qp of the no-carry product q p (a literal p: ordinary rows (sum_k p_k q_{j-k}) * 1 = qp_j ; p in witness columns: the rows of
    _product_rows, a second block), the 2l - 2 carries, one unknown each in  (P_j - qp_j - rem_j + carry_{j-1}) * 1 = 2^n carry_j , and the
    closing check row of limb 2l - 2, which has no carry to name."""

    def _modmul(self, cs, x, x_v, y, y_v, p_v, p=None):
        """-> (rem variables, rem values).  x, y: variables and values of the operands' limbs; p_v: the modulus' limbs, p: its
        variables where it is a witness"""
        one, r, n, l = ConstraintSystem.ONE, cs.r, self.n, self.limbs
        P_v, q_v, rem_v, qp_v, carry_v = modmul_values(x_v, y_v, p_v, n, r)
        P = [cs.new_witness_variable(v) for v in P_v]
        _product_rows(cs, x, y, P, 1)
        q = [cs.new_witness_variable(v) for v in q_v]
        rem = [cs.new_witness_variable(v) for v in rem_v]
        if self.decompose:
            for var, value in zip(q + rem, q_v + rem_v):
                cs.enforce_constraint([(1, var)], [(1, one)], _weighted(_new_bits(cs, value, n)))
        qp = [cs.new_witness_variable(v) for v in qp_v]
        if p is None:
            for j in range(2 * l - 1):
                cs.enforce_constraint([(p_v[j - i] % r, q[i]) for i in range(l) if 0 <= j - i < l and p_v[j - i]], [(1, one)], [(1, qp[j])])
        else:
            _product_rows(cs, q, p, qp, 1)
        carries = [cs.new_witness_variable(v) for v in carry_v]
        for j in range(2 * l - 1):
            lc = [(1, P[j]), (-1, qp[j])] + ([(-1, rem[j])] if j < l else []) + ([(1, carries[j - 1])] if j else [])
            cs.enforce_constraint(lc, [(1, one)], [(pow(2, n, r), carries[j])] if j < 2 * l - 2 else [])
        return rem, rem_v

    def _width(self):
        """the witnesses of one multiplication: P, q, rem, the bits, qp, the carries"""
        l = self.limbs
        return (2 * l - 1) + 2 * l + (2 * l * self.n if self.decompose else 0) + (2 * l - 1) + (2 * l - 2)

    def _hint(self, m0, at, p_cols=None):
        """the long division of the multiplication whose witnesses begin at witness index `at`; m0: the instance's length, which a
        witness index is offset by to give its CSR column"""
        l, first = self.limbs, m0 + at
        hint = {"n": self.n, "q": list(range(first + 2 * l - 1, first + 3 * l - 1)), "rem": list(range(first + 3 * l - 1, first + 4 * l - 1)),
                "D": list(range(first, first + 2 * l - 1))}
        if p_cols is None:
            hint["literal"] = int_limbs(self.modulus, self.n, l)
        else:
            hint["E"] = list(p_cols)
        if getattr(self, "wide", False):          # the wide long division (opcode 5): the same lists, first in the dict
            hint = dict([("op", "longdiv_wide")] + list(hint.items()))
        return hint


class LimbModMul(_PartialModMul):
    """Non-native modular multiplication (circom-bigint's BigMultModP, ark-r1cs-std's mul + reduce): per pair (a, b) of integers the
    given limbs of a and of b, the multiplication a b mod `modulus` of _PartialModMul with a literal modulus, and one ordinary row
    (sum rem_i) * 1 = s ; the public input is sum s.  The caller chooses a and b; the product limbs are a linear block, q and rem are
    the outputs of the declared hint (hints()), and everything else follows by ordinary rows and decompositions.  l max(a_i) max(b_i)
    must stay below r (modmul_values asserts it): the hint's dividend is the integer of the product limbs."""

    def __init__(self, pairs, modulus, n, limbs, decompose=True, wide=False):
        self.pairs, self.modulus, self.n, self.limbs, self.decompose = [(int(a), int(b)) for a, b in pairs], int(modulus), n, limbs, decompose
        self.wide = wide

    def hints(self, m0=2):
        """the declaration for Polymath.set_hints / api.encode_hints: one long division per pair, with the modulus as a literal;
        wide: the wide long division (RSA-2048 sizes)"""
        per = 2 * self.limbs + self._width() + 1
        return [self._hint(m0, i * per + 2 * self.limbs) for i in range(len(self.pairs))]

    def generate_constraints(self, cs):
        self._chosen = []
        one, n, l = ConstraintSystem.ONE, self.n, self.limbs
        p_v = int_limbs(self.modulus, n, l)
        total, total_v = [], 0
        for a_int, b_int in self.pairs:
            a_v, b_v = int_limbs(a_int, n, l), int_limbs(b_int, n, l)
            a = [self._given(cs, v) for v in a_v]
            b = [self._given(cs, v) for v in b_v]
            rem, rem_v = self._modmul(cs, a, a_v, b, b_v, p_v)
            s = cs.new_witness_variable(sum(rem_v))
            cs.enforce_constraint([(1, v) for v in rem], [(1, one)], [(1, s)])
            total.append((1, s))
            total_v += sum(rem_v)
        out = cs.new_input_variable(total_v)
        cs.enforce_constraint(total, [(1, one)], [(1, out)])

    def native(self, r):
        """-> (instance, witness) on Python integers, without generating a row; rem is (a b) mod modulus by Python's divmod"""
        n, l = self.n, self.limbs
        p_v = int_limbs(self.modulus, n, l)
        witness, total = [], 0
        for a_int, b_int in self.pairs:
            a_v, b_v = int_limbs(a_int, n, l), int_limbs(b_int, n, l)
            P, q, rem, qp, carries = modmul_values(a_v, b_v, p_v, n, r)
            assert limbs_int(rem, n) == a_int * b_int % self.modulus
            bits = [(v >> i) & 1 for v in q + rem for i in range(n)] if self.decompose else []
            witness += a_v + b_v + P + q + rem + bits + qp + carries + [sum(rem) % r]
            total += sum(rem)
        return [1, total % r], witness


class ModMulChain(_PartialModMul):
    """x_{t+1} = x_t b mod p for `steps` steps on l limbs of n bits: x_0 and b given, p a literal or -- witness_modulus -- l more given
    witnesses (the divisor of every hint is then its columns, and q p a second linear block per step); per step the multiplication of
    _PartialModMul, whose rem is x_{t+1}, and  (sum rem_i) * 1 = s_t ; the public input is sum s_t.  Blocks, hints, decompositions and
    carry rows alternate over 4 levels a step."""

    def __init__(self, x0, b, modulus, n, limbs, steps, witness_modulus=False, decompose=True, wide=False):
        self.x0, self.b, self.modulus, self.n, self.limbs, self.steps = int(x0), int(b), int(modulus), n, limbs, steps
        self.witness_modulus, self.decompose, self.wide = witness_modulus, decompose, wide

    def hints(self, m0=2):
        """the declaration for Polymath.set_hints / api.encode_hints: one long division per step, its divisor the literal modulus or
        the modulus' witness columns"""
        l = self.limbs
        head = 3 * l if self.witness_modulus else 2 * l
        p_cols = range(m0 + 2 * l, m0 + 3 * l) if self.witness_modulus else None
        return [self._hint(m0, head + t * (self._width() + 1), p_cols) for t in range(self.steps)]

    def generate_constraints(self, cs):
        self._chosen = []
        one, n, l = ConstraintSystem.ONE, self.n, self.limbs
        x_v, b_v, p_v = int_limbs(self.x0, n, l), int_limbs(self.b, n, l), int_limbs(self.modulus, n, l)
        x = [self._given(cs, v) for v in x_v]
        b = [self._given(cs, v) for v in b_v]
        p = [self._given(cs, v) for v in p_v] if self.witness_modulus else None
        total, total_v = [], 0
        for _ in range(self.steps):
            x, x_v = self._modmul(cs, x, x_v, b, b_v, p_v, p)
            s = cs.new_witness_variable(sum(x_v))
            cs.enforce_constraint([(1, v) for v in x], [(1, one)], [(1, s)])
            total.append((1, s))
            total_v += sum(x_v)
        out = cs.new_input_variable(total_v)
        cs.enforce_constraint(total, [(1, one)], [(1, out)])

    def native(self, r):
        """-> (instance, witness) on Python integers, without generating a row; x_t = x_0 b^t mod p by Python's pow"""
        n, l = self.n, self.limbs
        x_v, b_v, p_v = int_limbs(self.x0, n, l), int_limbs(self.b, n, l), int_limbs(self.modulus, n, l)
        witness, total = x_v + b_v + (p_v if self.witness_modulus else []), 0
        for t in range(self.steps):
            P, q, rem, qp, carries = modmul_values(x_v, b_v, p_v, n, r)
            assert limbs_int(rem, n) == self.x0 * pow(self.b, t + 1, self.modulus) % self.modulus
            bits = [(v >> i) & 1 for v in q + rem for i in range(n)] if self.decompose else []
            witness += P + q + rem + bits + qp + carries + [sum(rem) % r]
            total += sum(rem)
            x_v = rem
        return [1, total % r], witness


class RsaVerify(_PartialModMul):
    """The arithmetic of an RSA signature check with the public exponent 2^squarings + 1 (65537 by default) on l limbs of n bits:
    x_0 = s given, x_{t+1} = x_t^2 mod N `squarings` times, then y = x_last s mod N; every step is the multiplication of
    _PartialModMul (a squaring passes the same limbs twice) and the public input is the sum of y's limbs.  N is a literal or --
    witness_modulus -- l more given witnesses.  The dividends have about twice the modulus' bits, so hints() declares the WIDE long
    division.  Both RSA-2048 shapes keep every no-carry product limb below r on both curves: 32 limbs of 64 bits (32 * 2^128) and the
    zk-email circuits' 17 limbs of 121 bits (17 * 2^242 < 2^247)."""

    wide = True

    def __init__(self, signature, modulus, n, limbs, squarings=16, witness_modulus=False, decompose=False):
        self.signature, self.modulus, self.n, self.limbs, self.squarings = int(signature), int(modulus), n, limbs, squarings
        self.witness_modulus, self.decompose = witness_modulus, decompose

    def hints(self, m0=2):
        """one wide long division per multiplication, its divisor the literal modulus or the modulus' witness columns"""
        l = self.limbs
        head = 2 * l if self.witness_modulus else l
        p_cols = range(m0 + l, m0 + 2 * l) if self.witness_modulus else None
        return [self._hint(m0, head + t * self._width(), p_cols) for t in range(self.squarings + 1)]

    def generate_constraints(self, cs):
        self._chosen = []
        one, n, l = ConstraintSystem.ONE, self.n, self.limbs
        s_v, p_v = int_limbs(self.signature, n, l), int_limbs(self.modulus, n, l)
        s = [self._given(cs, v) for v in s_v]
        p = [self._given(cs, v) for v in p_v] if self.witness_modulus else None
        x, x_v = s, s_v
        for _ in range(self.squarings):
            x, x_v = self._modmul(cs, x, x_v, x, x_v, p_v, p)
        y, y_v = self._modmul(cs, x, x_v, s, s_v, p_v, p)
        out = cs.new_input_variable(sum(y_v))
        cs.enforce_constraint([(1, v) for v in y], [(1, one)], [(1, out)])

    def native(self, r):
        """-> (instance, witness) on Python integers, without generating a row; y = s^(2^squarings + 1) mod N by Python's pow"""
        n, l = self.n, self.limbs
        s_v, p_v = int_limbs(self.signature, n, l), int_limbs(self.modulus, n, l)
        witness, x_v = s_v + (p_v if self.witness_modulus else []), s_v
        for t in range(self.squarings + 1):
            P, q, rem, qp, carries = modmul_values(x_v, x_v if t < self.squarings else s_v, p_v, n, r)
            bits = [(v >> i) & 1 for v in q + rem for i in range(n)] if self.decompose else []
            witness += P + q + rem + bits + qp + carries
            x_v = rem
        assert limbs_int(x_v, n) == pow(self.signature, 2 ** self.squarings + 1, self.modulus)
        return [1, sum(x_v) % r], witness


class LimbDivision(_Partial):
    """The wide long division's test rig: per case (D limbs, E limbs) -- given as they are: a limb may be anything below r, limbs
    need not be normalised -- kq quotient limbs and kr remainder limbs of n bits that ONLY the declared hint determines (hints():
    opcode 5, or opcode 1 with wide=False), and one ordinary row  (sum q_i + sum rem_i) * 1 = s ; the public input is sum s.
    divisor="literal" puts the divisor's limbs into the hint instead of into witness columns.  No row checks the division: the rig
    is for comparing the solver with Python's divmod, which native() is.  native() refuses a case that the solver would report stuck
    (E = 0, D >= 2^8192, E >= 2^4096, a quotient or remainder that does not fit) unless stuck=True, and then stores zeros."""

    def __init__(self, cases, n, kq, kr, divisor="columns", wide=True, stuck=False):
        assert divisor in ("columns", "literal")
        self.cases = [([int(v) for v in D], [int(v) for v in E]) for D, E in cases]
        self.n, self.kq, self.kr, self.divisor, self.wide, self.stuck = n, kq, kr, divisor, wide, stuck

    def _outputs(self, D, E):
        """-> (q limbs, rem limbs, stuck)"""
        n, kq, kr = self.n, self.kq, self.kr
        d_bits, e_bits = (8192, 4096) if self.wide else (1024, 512)
        Dv, Ev = limbs_int(D, n), limbs_int(E, n)
        bad = Ev == 0 or Dv >= 1 << d_bits or Ev >= 1 << e_bits
        if not bad:
            q, rem = divmod(Dv, Ev)
            bad = q >= 1 << (n * kq) or rem >= 1 << (n * kr)
        if bad:
            assert self.stuck, "the case is stuck: D = %d bits, E = %d bits" % (Dv.bit_length(), Ev.bit_length())
            return [0] * kq, [0] * kr, True
        return int_limbs(q, n, kq), int_limbs(rem, n, kr), False

    def stuck_cases(self):
        """which cases the solver reports stuck"""
        return [self._outputs(D, E)[2] for D, E in self.cases]

    def _columns(self, m0=2):
        """per case the CSR columns (D, E, q, rem); E is empty for a literal divisor"""
        at, out = m0, []
        for D, E in self.cases:
            kE = len(E) if self.divisor == "columns" else 0
            d = list(range(at, at + len(D)))
            e = list(range(at + len(D), at + len(D) + kE))
            q = list(range(e[-1] + 1 if e else d[-1] + 1, (e[-1] + 1 if e else d[-1] + 1) + self.kq))
            rem = list(range(q[-1] + 1, q[-1] + 1 + self.kr))
            out.append((d, e, q, rem))
            at = rem[-1] + 2          # and s
        return out

    def hints(self, m0=2):
        out = []
        for (D, E), (d, e, q, rem) in zip(self.cases, self._columns(m0)):
            hint = {"op": "longdiv_wide"} if self.wide else {}
            hint.update({"n": self.n, "q": q, "rem": rem, "D": d})
            if self.divisor == "columns":
                hint["E"] = e
            else:
                hint["literal"] = list(E)
            out.append(hint)
        return out

    def generate_constraints(self, cs):
        self._chosen = []
        one = ConstraintSystem.ONE
        total, total_v = [], 0
        for D, E in self.cases:
            q_v, rem_v, _ = self._outputs(D, E)
            for v in D + (E if self.divisor == "columns" else []):
                self._given(cs, v)
            outs = [cs.new_witness_variable(v) for v in q_v + rem_v]
            s = cs.new_witness_variable(sum(q_v + rem_v) % cs.r)
            cs.enforce_constraint([(1, v) for v in outs], [(1, one)], [(1, s)])
            total.append((1, s))
            total_v += sum(q_v + rem_v)
        out = cs.new_input_variable(total_v % cs.r)
        cs.enforce_constraint(total, [(1, one)], [(1, out)])

    def native(self, r):
        """-> (instance, witness) on Python integers: Python's divmod"""
        witness, total = [], 0
        for D, E in self.cases:
            q_v, rem_v, _ = self._outputs(D, E)
            witness += D + (E if self.divisor == "columns" else []) + q_v + rem_v + [sum(q_v + rem_v) % r]
            total += sum(q_v + rem_v)
        return [1, total % r], witness


def rsa_modulus(bits=2048, seed=SPLITMIX_SEED):
    """an odd integer of exactly `bits` bits drawn from SplitMix64(seed) (no prime product: the arithmetic does not ask for one) and a
    signature below it"""
    g = SplitMix64(seed)
    draw = lambda: sum(g.next_u64() << (64 * i) for i in range(-(-bits // 64))) & ((1 << bits) - 1)
    modulus = draw() | 1 | 1 << (bits - 1)
    return modulus, draw() % modulus


def division_cases(n, kD, kE, r, seed=SPLITMIX_SEED):
    """The operand families of the wide long division for LimbDivision(cases, n, kD, kE), each where it fits the shape: -> a list of
    (name, D limbs, E limbs), none of them stuck.  Values are cut into normalised limbs unless the name says otherwise.  The word
    counts m are those of the divisor in base 2^32: lane and half-wave edges of the kernel.  The ADD-BACK family
    E = 2^(32 m - 1) + 1, D = ((E - 1) << 32 k) | 3 makes algorithm D's estimate one too large, the SATURATING family
    E = (0xFFFFFFFF << 32 (m - 1)) | 5, D = (E << 32) - 1 makes its first estimate reach 2^32: random operands do neither."""
    g = SplitMix64(seed)
    Dbits, Ebits = min(n * kD, 8192), min(n * kE, 4096)
    rnd = lambda bits: (sum(g.next_u64() << (64 * i) for i in range(-(-bits // 64))) & ((1 << bits) - 1)) if bits > 0 else 0
    exact = lambda bits: rnd(bits - 1) | 1 << (bits - 1)              # exactly `bits` bits
    out = []

    def add(name, D, E, d_limbs=None, e_limbs=None):
        if E <= 0 or D < 0 or D >= 1 << Dbits or E >= 1 << Ebits:
            return
        out.append((name, d_limbs or int_limbs(D, n, kD), e_limbs or int_limbs(E, n, kE)))

    add("random", rnd(Dbits), exact(Ebits))
    add("random, a divisor of half the width", exact(Dbits), exact(max(1, Ebits // 2)))
    add("a divisor of one significant word", rnd(Dbits), exact(min(32, Ebits)))
    add("a divisor of one significant word, small", rnd(Dbits), 3)
    for m in (2, 3, 63, 64, 65, 127, 128):
        if 32 * m <= Ebits:
            add("a divisor of %d significant words" % m, rnd(Dbits), exact(32 * m - (g.next_u64() % 32)))
    top = max(1, Ebits // 32)
    if Ebits >= 32:
        add("normalising shift 0", rnd(Dbits), exact(32 * top))
        add("normalising shift 31", rnd(Dbits), rnd(32 * (top - 1)) | 1 << (32 * (top - 1)))
    for m in (3, 64, 65, 128):
        E = (1 << (32 * m - 1)) + 1
        for k in (1, 2, 3):
            add("add-back m = %d k = %d" % (m, k), ((E - 1) << (32 * k)) | 3, E)
        E = (0xFFFFFFFF << (32 * (m - 1))) | 5
        add("saturating m = %d" % m, (E << 32) - 1, E)
    E = exact(Ebits)
    add("D < E", rnd(max(0, Ebits - 1)), E)
    add("D = 0", 0, E)
    add("D = E", E, E)
    add("D = E - 1", E - 1, E)
    add("E = 1", rnd(Dbits), 1)
    if Dbits == 8192 and Ebits == 4096:
        add("E = 2^4096 - 1 under D = 2^8192 - 1", (1 << 8192) - 1, (1 << 4096) - 1)
    add("the largest operands of the shape", (1 << Dbits) - 1, (1 << Ebits) - 1)
    # every limb r - 1, so that every word of the sum carries: kD limbs of the dividend where that stays below 2^8192 and the quotient
    # fits, the divisor's limbs where the remainder still fits kE limbs of n bits
    rbits = r.bit_length()
    d_full = [r - 1] * kD
    e_count = max(k for k in range(0, kE + 1) if k == 0 or n * (k - 1) + rbits <= n * kE)
    if limbs_int(d_full, n) < 1 << 8192 and n * (kD - 1) + rbits <= n * kD + Ebits - 1:
        add("every dividend limb r - 1", 0, E, d_limbs=d_full)
        if e_count:
            e_full = [r - 1] * e_count
            if limbs_int(d_full, n) // limbs_int(e_full, n) < 1 << (n * kD):
                out.append(("every limb r - 1", d_full, e_full))
    return out


def modmul_pairs(modulus, count, seed=SPLITMIX_SEED, bits=None):
    """`count` pairs of integers below `modulus` (or below 2^bits) for LimbModMul, drawn from SplitMix64(seed)"""
    g = SplitMix64(seed)
    draw = lambda: sum(g.next_u64() << (64 * i) for i in range(-(-modulus.bit_length() // 64))) % (modulus if bits is None else 1 << bits)
    return [(draw(), draw()) for _ in range(count)]


def subtraction_pad(modulus, n, limbs, operand_bits=None):
    """THE PADDING CONSTANT of limb-wise subtraction modulo `modulus`: `limbs` limbs whose integer  sum pad_j 2^(n j)  is a multiple of
    the modulus and each of which is at least 2^operand_bits - 1, so that  x_j - y_j + pad_j  is a non-negative integer for every
    subtrahend limb y_j < 2^operand_bits and the sum is x - y modulo the modulus.  With operand_bits = n (the default) it is
    pad_j = 2^n + e_j for e the n-bit limbs of  -(sum 2^n 2^(n j)) mod modulus : every limb in [2^n, 2^(n + 1)).  With narrower
    operands (limbs so wide that a product of two full limbs would pass r) the pad must be narrow too, and there is no such multiple
    in general; the modulus' own limbs serve where each is at least 2^operand_bits - 1, and anything else is refused."""
    operand_bits = n if operand_bits is None else operand_bits
    if operand_bits == n:
        base = sum(1 << (n * (j + 1)) for j in range(limbs))
        pad = [(1 << n) + e for e in int_limbs(-base % modulus, n, limbs)]
    else:
        pad = int_limbs(modulus, n, limbs)
        assert all(v >= (1 << operand_bits) - 1 for v in pad), "no narrow pad: a limb of the modulus is below 2^operand_bits - 1"
    assert limbs_int(pad, n) % modulus == 0 and all(v >= (1 << operand_bits) - 1 for v in pad)
    return pad


class _ValuesOnly:
    """A ConstraintSystem's variables and values without its rows: what native() runs a generator on"""

    def __init__(self, r):
        self.r, self.instance, self.witness = r, [1], []

    new_input_variable = ConstraintSystem.new_input_variable
    new_witness_variable = ConstraintSystem.new_witness_variable

    def enforce_constraint(self, a, b, c):
        pass


_LAYOUT_R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001   # BN254's r, the smaller one: hints() lays a circuit out on it


class _PartialModDiv(_Partial):
    """What LimbModDiv and EcAddChain share: arithmetic modulo a foreign `modulus` on l limbs of n bits whose divisions are declared
    hints.  A LIMB here is (lc, value, bound): a linear combination of variables, its value as a Python integer (never negative, never
    reduced mod r) and an upper bound of that value over all inputs; the bounds prove that no limb can reach r (asserted), so that
    int(column) is the integer the hints are specified on.
      _quotient   Z = (N+ - N-) / (D+ - D-) mod p from a MODULAR hint: l witnesses, with `decompose` their bits
      _product    the 2l - 1 limbs of a no-carry product, pinned at the points 1 .. 2l - 1: a linear block
      _reduce     T mod p for limbs T from a LONG-DIVISION hint: a column per limb of T that is not one already (an ordinary row),
                  the limbs of q and rem (hinted; with `decompose` their bits), the limbs of the no-carry product q p (ordinary rows:
                  p is a literal), and the carries of  T_j - qp_j - rem_j + carry_{j-1} = carry_j 2^n  with the closing check row.
                  With `zero` the remainder must be zero -- the division is exact: asserted on the values, and l check rows
                  rem_j * 1 = 0  pin the hint-owned remainder columns
    Subtractions add subtraction_pad(), so every dividend limb stays a non-negative integer."""

    def _setup(self, cs):
        self._chosen, self._declared = [], []
        self._pad = subtraction_pad(self.modulus, self.n, self.limbs, self.operand_bits)

    def _given_limbs(self, cs, value, bits=None):
        bits = self.n if bits is None else bits
        values = int_limbs(value, self.n, self.limbs)
        assert all(v < 1 << bits for v in values), "an operand limb is wider than operand_bits"
        return [([(1, self._given(cs, v))], v, (1 << bits) - 1) for v in values]

    def _minus(self, x, y, scale=1):
        """x - y + scale pad, limb by limb; y may be shorter than x (its missing limbs are zero and take no pad)"""
        out = []
        for j, (lc, v, hi) in enumerate(x):
            if j < len(y):
                pad = scale * self._pad[j]
                assert y[j][2] <= pad, "a subtrahend limb may exceed the pad"
                lc = [term for term in _merged(lc + [(-c, var) for c, var in y[j][0]] + [(pad, ConstraintSystem.ONE)]) if term[0]]
                v, hi = v - y[j][1] + pad, hi + pad
            assert v >= 0
            out.append((lc, v, hi))
        return out

    def _bits(self, cs, limbs):
        if self.decompose:
            for lc, v, _ in limbs:
                cs.enforce_constraint(lc, [(1, ConstraintSystem.ONE)], _weighted(_new_bits(cs, v, self.n)))

    def _fresh(self, cs, values):
        first = len(cs.witness)
        return [([(1, cs.new_witness_variable(v))], v, (1 << self.n) - 1) for v in values], list(range(first, first + len(values)))

    def _quotient(self, cs, Np, Nm, Dp, Dm):
        """Operands: lists of limbs that are single witness columns (or empty lists).  -> the limbs of Z"""
        p, n = self.modulus, self.n
        index = lambda limbs: [lc[0][1][1] for lc, _, _ in limbs]
        assert all(len(lc) == 1 and lc[0][0] == 1 and lc[0][1][0] == "wit" for lc, _, _ in Np + Nm + Dp + Dm)
        value = lambda limbs: limbs_int([v for _, v, _ in limbs], n)
        N = (value(Np) - value(Nm)) % p if Np or Nm else 1
        D = (value(Dp) - value(Dm)) % p
        Z = N * pow(D, -1, p) % p            # raises where D has no inverse: the generator's inputs must avoid it
        out, at = self._fresh(cs, int_limbs(Z, n, self.limbs))
        self._declared.append({"op": "moddiv", "n": n, "z": at, "Np": index(Np), "Nm": index(Nm), "Dp": index(Dp), "Dm": index(Dm),
                               "literal": int_limbs(p, n, self.limbs)})
        self._bits(cs, out)
        return out

    def _product(self, cs, a, b):
        r = cs.r
        values = [sum(a[i][1] * b[j - i][1] for i in range(len(a)) if 0 <= j - i < len(b)) for j in range(len(a) + len(b) - 1)]
        bounds = [sum(a[i][2] * b[j - i][2] for i in range(len(a)) if 0 <= j - i < len(b)) for j in range(len(a) + len(b) - 1)]
        assert max(bounds) < r, "a limb of the no-carry product may reach r"
        out = [([(1, cs.new_witness_variable(v))], v, hi) for v, hi in zip(values, bounds)]
        at = lambda limbs, c: _merged([(coef * pow(c, i, r), var) for i, (lc, _, _) in enumerate(limbs) for coef, var in lc])
        for c in range(1, len(out) + 1):
            cs.enforce_constraint(at(a, c), at(b, c), at(out, c))
        return out

    def _reduce(self, cs, T, zero=False):
        one, r, n, l, p = ConstraintSystem.ONE, cs.r, self.n, self.limbs, self.modulus
        assert max(hi for _, _, hi in T) < r, "a dividend limb may reach r"
        cols = []
        for lc, v, hi in T:
            if not (len(lc) == 1 and lc[0][0] == 1 and lc[0][1][0] == "wit"):
                var = cs.new_witness_variable(v)
                cs.enforce_constraint(lc, [(1, one)], [(1, var)])
                lc = [(1, var)]
            cols.append((lc, v, hi))
        top = limbs_int([hi for _, _, hi in T], n)
        assert top < 1 << 1024, "the dividend may reach 2^1024"
        kq = max(1, -(-(top // p).bit_length() // n))
        q_int, rem_int = divmod(limbs_int([v for _, v, _ in T], n), p)
        assert not zero or rem_int == 0, "a hinted division that must be exact is not"
        q, q_at = self._fresh(cs, int_limbs(q_int, n, kq))
        rem, rem_at = self._fresh(cs, int_limbs(rem_int, n, l))
        self._declared.append({"n": n, "q": q_at, "rem": rem_at, "D": [lc[0][1][1] for lc, _, _ in cols], "literal": int_limbs(p, n, l)})
        self._bits(cs, q + rem)
        p_v = int_limbs(p, n, l)
        width = max(len(cols), kq + l - 1)
        qp_v = [sum(q[i][1] * p_v[j - i] for i in range(kq) if 0 <= j - i < l) for j in range(width)]
        assert max(qp_v) < r
        qp = [cs.new_witness_variable(v) for v in qp_v]
        for j in range(width):
            cs.enforce_constraint([(p_v[j - i] % r, q[i][0][0][1]) for i in range(kq) if 0 <= j - i < l and p_v[j - i]], [(1, one)], [(1, qp[j])])
        carries, carry = [], 0
        for j in range(width):
            total = (cols[j][1] if j < len(cols) else 0) - qp_v[j] - (rem[j][1] if j < l else 0) + carry
            assert total % (1 << n) == 0
            carry = total >> n
            lc = (cols[j][0] if j < len(cols) else []) + [(-1, qp[j])] + ([(-1, rem[j][0][0][1])] if j < l else []) + ([(1, carries[-1])] if j else [])
            if j < width - 1:
                carries.append(cs.new_witness_variable(carry))
            cs.enforce_constraint(lc, [(1, one)], [(pow(2, n, r), carries[-1])] if j < width - 1 else [])
        assert carry == 0
        if zero:
            for lc, _, _ in rem:
                cs.enforce_constraint(lc, [(1, one)], [])
        return rem

    def _close(self, cs, sums):
        """one ordinary row per list of limbs,  (sum limbs) * 1 = s , and the public input  sum s"""
        one, total, total_v = ConstraintSystem.ONE, [], 0
        for limbs in sums:
            v = sum(value for _, value, _ in limbs)
            s = cs.new_witness_variable(v)
            cs.enforce_constraint(_merged([term for lc, _, _ in limbs for term in lc]), [(1, one)], [(1, s)])
            total.append((1, s))
            total_v += v
        out = cs.new_input_variable(total_v)
        cs.enforce_constraint(total, [(1, one)], [(1, out)])

    def hints(self, m0=2):
        """the declaration for Polymath.set_hints / api.encode_hints: the modular and the long-division hints in the order the
        generator meets them, the modulus a literal in all of them.  The witness indices are those of the generator's last pass
        (generate_constraints, partial or native; they depend neither on r nor on the values), so a generator that was run as part of
        a larger system declares its columns there"""
        if not getattr(self, "_declared", None):     # no generate_constraints, partial or native yet: a pass for the layout alone
            self.generate_constraints(_ValuesOnly(_LAYOUT_R))
        return [{key: v if key in ("op", "n", "literal") else [m0 + j for j in v] for key, v in hint.items()} for hint in self._declared]

    def native(self, r):
        """-> (instance, witness) on Python integers, without generating a row; every value comes from Python's pow and divmod, and
        every division that must be exact is asserted to be"""
        cs = _ValuesOnly(r)
        self.generate_constraints(cs)
        return cs.instance, cs.witness


class LimbModDiv(_PartialModDiv):
    """Non-native modular division (the slope of a point addition, ark-r1cs-std's non-native inverse, circom-ecdsa's BigModInv): per
    case (N+, N-, D+, D-) of integers their given limbs, Z = (N+ - N-) / (D+ - D-) mod `modulus` from a modular hint, and the check
    Z (D+ - D- + pad) - (N+ - N-) + pad = 0 (mod modulus): the product's block, then _reduce with a remainder that must be zero.  A
    case (None, None, D+, D-) is the inverse: N = 1, no numerator columns.  One ordinary row per case sums Z's limbs, and the public
    input is the sum of those.  operand_bits < n keeps the given limbs and the pad narrow, for limbs so wide that full ones would
    carry a product past r (n = 128): see subtraction_pad."""

    def __init__(self, cases, modulus, n, limbs, decompose=True, operand_bits=None):
        self.cases, self.modulus, self.n, self.limbs, self.decompose, self.operand_bits = [tuple(c) for c in cases], int(modulus), n, limbs, decompose, operand_bits

    def generate_constraints(self, cs):
        self._setup(cs)
        sums = []
        for Np_v, Nm_v, Dp_v, Dm_v in self.cases:
            inverse = Np_v is None and Nm_v is None
            Np, Nm = ([], []) if inverse else (self._given_limbs(cs, Np_v, self.operand_bits), self._given_limbs(cs, Nm_v, self.operand_bits))
            Dp, Dm = self._given_limbs(cs, Dp_v, self.operand_bits), self._given_limbs(cs, Dm_v, self.operand_bits)
            Z = self._quotient(cs, Np, Nm, Dp, Dm)
            T = self._product(cs, Z, self._minus(Dp, Dm))
            numerator = [([(1, ConstraintSystem.ONE)], 1, 1)] + [([], 0, 0)] * (self.limbs - 1) if inverse else self._minus(Np, Nm)
            # Z D - N + pad, the whole pad: a numerator N+ - N- + pad carries one pad itself, so its subtraction takes two
            self._reduce(cs, self._minus(T, numerator, 2 if not inverse else 1), zero=True)
            sums.append(Z)
        self._close(cs, sums)


class EcAddChain(_PartialModDiv):
    """`steps` affine additions R <- R + Q on a short Weierstrass curve y^2 = x^3 + b over `modulus` (b plays no part in an addition
    of points with different x), on l limbs of n bits: R_0 = `point` and Q = `addend` are given, and the caller keeps the
    x-coordinates of R_t and Q distinct (asserted).  Per step
        lambda = (Y2 - Y1) / (X2 - X1)          a modular hint
        lambda (X2 - X1) - (Y2 - Y1) = 0        the product's block, _reduce to zero
        X3 = lambda^2 - X1 - X2                 the product's block, _reduce
        Y3 = lambda (X1 - X3) - Y1              the product's block, _reduce
    all modulo the modulus, so modular and long-division hints alternate through the dependency levels.  One ordinary row per step sums
    the limbs of X3 and Y3; the public input is the sum of those.  The result is compared with affine addition on Python integers."""

    def __init__(self, point, addend, modulus, n, limbs, steps, decompose=True):
        self.point, self.addend, self.modulus, self.n, self.limbs, self.steps = tuple(point), tuple(addend), int(modulus), n, limbs, steps
        self.decompose, self.operand_bits = decompose, None

    def result(self):
        """R_0 + steps Q by the affine formulas on Python integers"""
        p, (x1, y1), (x2, y2) = self.modulus, self.point, self.addend
        for _ in range(self.steps):
            assert (x1 - x2) % p, "the x-coordinates meet: the chord's slope is not defined"
            lam = (y2 - y1) * pow(x2 - x1, -1, p) % p
            x3 = (lam * lam - x1 - x2) % p
            x1, y1 = x3, (lam * (x1 - x3) - y1) % p
        return x1, y1

    def generate_constraints(self, cs):
        self._setup(cs)
        n, want = self.n, self.result()         # asserts that every chord has a slope
        X1, Y1 = self._given_limbs(cs, self.point[0]), self._given_limbs(cs, self.point[1])
        X2, Y2 = self._given_limbs(cs, self.addend[0]), self._given_limbs(cs, self.addend[1])
        sums = []
        for _ in range(self.steps):
            lam = self._quotient(cs, Y2, Y1, X2, X1)
            dY = self._minus(Y2, Y1)
            self._reduce(cs, self._minus(self._product(cs, lam, self._minus(X2, X1)), dY, 2), zero=True)
            X3 = self._reduce(cs, self._minus(self._minus(self._product(cs, lam, lam), X1), X2))
            Y3 = self._reduce(cs, self._minus(self._product(cs, lam, self._minus(X1, X3)), Y1))
            sums.append(X3 + Y3)
            X1, Y1 = X3, Y3
        assert (limbs_int([v for _, v, _ in X1], n), limbs_int([v for _, v, _ in Y1], n)) == want
        self._close(cs, sums)


def moddiv_cases(modulus, count, seed=SPLITMIX_SEED, inverses=0, narrow=None):
    """`count` cases (N+, N-, D+, D-) of integers for LimbModDiv, drawn from SplitMix64(seed), the last `inverses` of them
    (None, None, D+, D-).  The operands are below `modulus`, or -- narrow = (n, limbs, bits) -- have `limbs` limbs of n bits of which
    only the low `bits` are drawn (LimbModDiv's operand_bits).  A denominator without an inverse modulo a composite modulus is drawn
    again."""
    from math import gcd
    g = SplitMix64(seed)
    rnd = lambda bits: sum(g.next_u64() << (64 * i) for i in range(-(-bits // 64))) & ((1 << bits) - 1)
    draw = (lambda: rnd(modulus.bit_length() + 64) % modulus) if narrow is None else (lambda: sum(rnd(narrow[2]) << (narrow[0] * j) for j in range(narrow[1])))
    out = []
    while len(out) < count:
        Np, Nm, Dp, Dm = draw(), draw(), draw(), draw()
        if gcd((Dp - Dm) % modulus, modulus) == 1:
            out.append((None, None, Dp, Dm) if len(out) >= count - inverses else (Np, Nm, Dp, Dm))
    return out


def narrow_modulus(n, limbs, bits, seed=SPLITMIX_SEED):
    """An odd modulus (not a prime) whose `limbs` limbs of n bits each lie in [2^bits, 2^(bits + 1)): its own limbs are a narrow
    subtraction_pad for operands of `bits`-bit limbs"""
    g = SplitMix64(seed)
    return sum(((1 << bits) + (g.next_u64() | (1 if j == 0 else 0))) << (n * j) for j in range(limbs))


def product_pad(modulus, n, bounds):
    """subtraction_pad for subtrahends whose limbs are not n-bit ones -- the 2l - 1 limbs of a no-carry product, scaled or not:
    len(bounds) limbs whose integer  sum pad_j 2^(n j)  is a multiple of the modulus and pad_j >= bounds[j], the largest value limb j
    of the subtrahend can take.  pad_j = 2^(b_j) + e_j with 2^(b_j) the smallest power of two above bounds[j] and e the n-bit limbs of
    -(sum 2^(b_j) 2^(n j)) mod modulus, laid over the lowest limbs (more of them than the subtrahend has are appended)."""
    tops = [1 << int(hi).bit_length() for hi in bounds]
    e = -sum(t << (n * j) for j, t in enumerate(tops)) % modulus
    count = max(len(tops), -(-max(e.bit_length(), 1) // n))
    pad = [(tops[j] if j < len(tops) else 0) + v for j, v in enumerate(int_limbs(e, n, count))]
    assert limbs_int(pad, n) % modulus == 0 and all(v >= hi for v, hi in zip(pad, bounds))
    return pad


def affine_add(p, P1, P2):
    """P1 + P2 on y^2 = x^3 + b over the prime p (a = 0), affine on Python integers; None is the point at infinity"""
    if P1 is None or P2 is None:
        return P1 if P2 is None else P2
    (x1, y1), (x2, y2) = P1, P2
    if x1 == x2 and (y1 + y2) % p == 0:
        return None
    lam = 3 * x1 * x1 * pow(2 * y1, -1, p) % p if P1 == P2 else (y2 - y1) * pow(x2 - x1, -1, p) % p
    x3 = (lam * lam - x1 - x2) % p
    return x3, (lam * (x1 - x3) - y1) % p


def affine_mul(p, k, P1):
    """[k] P1 by double-and-add on Python integers"""
    out = None
    for bit in bin(k)[2:] if k else "":
        out = affine_add(p, out, out)
        if bit == "1":
            out = affine_add(p, out, P1)
    return out


class _PartialModMulDiv(_PartialModDiv):
    """What LimbModMulDiv, EcDoubleAddChain and EcdsaVerify add to _PartialModDiv: the MULTIPLY-DIVIDE hint (opcode 7), subtraction of
    product limbs, and a second modulus.
      _over       the helpers of _PartialModDiv read self.modulus and its pad; `with self._over(q):` runs them modulo q (ECDSA works
                  modulo the field's prime and modulo the group order)
      _muldiv     Z with cD (D+ - D-) Z = cN (A B + N+ - N-) mod p from a multiply-divide hint: l witnesses, with `decompose` their bits
      _scaled     c times a list of limbs
      _minus_wide x - y + product_pad(bounds of y): y may be the limbs of a product
      _double, _add   a tangent and a chord on y^2 = x^3 + b, each slope a hint with its exact check"""

    def _over(self, modulus):
        circuit = self

        class _Scope:
            def __enter__(self):
                self.saved = circuit.modulus, circuit._pad
                circuit.modulus, circuit._pad = modulus, subtraction_pad(modulus, circuit.n, circuit.limbs, circuit.operand_bits)

            def __exit__(self, *exc):
                circuit.modulus, circuit._pad = self.saved

        return _Scope()

    @staticmethod
    def _scaled(limbs, c):
        return [([(coef * c, var) for coef, var in lc], v * c, hi * c) for lc, v, hi in limbs]

    def _minus_wide(self, x, y):
        pad = product_pad(self.modulus, self.n, [hi for _, _, hi in y])
        zero = ([], 0, 0)
        out = []
        for j in range(max(len(x), len(pad))):
            (lc, v, hi), (lc_y, v_y, _) = x[j] if j < len(x) else zero, y[j] if j < len(y) else zero
            pad_j = pad[j] if j < len(pad) else 0
            lc = [term for term in _merged(lc + [(-c, var) for c, var in lc_y] + [(pad_j, ConstraintSystem.ONE)]) if term[0]]
            assert v - v_y + pad_j >= 0
            out.append((lc, v - v_y + pad_j, hi + pad_j))
        return out

    def _muldiv(self, cs, A, B, Np, Nm, Dp, Dm, cN=1, cD=1):
        """Operands: lists of limbs that are single witness columns (or empty lists); B may be A itself.  -> the limbs of Z"""
        p, n = self.modulus, self.n
        index = lambda limbs: [lc[0][1][1] for lc, _, _ in limbs]
        assert all(len(lc) == 1 and lc[0][0] == 1 and lc[0][1][0] == "wit" for lc, _, _ in A + B + Np + Nm + Dp + Dm)
        value = lambda limbs: limbs_int([v for _, v, _ in limbs], n)
        N = cN * (value(A) * value(B) + value(Np) - value(Nm)) % p
        D = cD * ((value(Dp) - value(Dm)) if Dp or Dm else 1) % p
        Z = N * pow(D, -1, p) % p            # raises where cD D has no inverse: the generator's inputs must avoid it
        out, at = self._fresh(cs, int_limbs(Z, n, self.limbs))
        self._declared.append({"op": "modmuldiv", "n": n, "z": at, "A": index(A), "B": index(B), "Np": index(Np), "Nm": index(Nm), "Dp": index(Dp), "Dm": index(Dm),
                               "cN": cN, "cD": cD, "literal": int_limbs(p, n, self.limbs)})
        self._bits(cs, out)
        return out

    def _muldiv_check(self, cs, Z, A, B, Np, Nm, Dp, Dm, cN=1, cD=1):
        """cD Z (D+ - D-) - cN (A B + N+ - N-) = 0 (mod p), exactly: the products' blocks, then _reduce with a remainder of zero"""
        if Dp or Dm:
            left = self._product(cs, Z, self._scaled(self._minus(Dp, Dm) if Dm else Dp, cD))
        else:
            left = self._scaled(Z, cD)
        right = self._product(cs, A, B)
        if Np or Nm:
            addend = self._minus(Np or [([], 0, 0)] * len(Nm), Nm) if Nm else Np
            right = [(_merged(lc + (addend[j][0] if j < len(addend) else [])), v + (addend[j][1] if j < len(addend) else 0), hi + (addend[j][2] if j < len(addend) else 0))
                     for j, (lc, v, hi) in enumerate(right)]
        self._reduce(cs, self._minus_wide(left, self._scaled(right, cN)), zero=True)

    def _double(self, cs, X, Y):
        """2 (X, Y): lambda = 3 X^2 / (2 Y) from the multiply-divide hint, the tangent check lambda 2 Y - 3 X X = 0, then
        X' = lambda^2 - 2 X and Y' = lambda (X - X') - Y"""
        lam = self._muldiv(cs, X, X, [], [], Y, [], 3, 2)
        self._muldiv_check(cs, lam, X, X, [], [], Y, [], 3, 2)
        X3 = self._reduce(cs, self._minus(self._minus(self._product(cs, lam, lam), X), X))
        Y3 = self._reduce(cs, self._minus(self._product(cs, lam, self._minus(X, X3)), Y))
        return X3, Y3

    def _add(self, cs, X1, Y1, X2, Y2):
        """(X1, Y1) + (X2, Y2) for X1 != X2, as EcAddChain does it: the chord's slope from a modular hint with its exact check"""
        lam = self._quotient(cs, Y2, Y1, X2, X1)
        self._reduce(cs, self._minus(self._product(cs, lam, self._minus(X2, X1)), self._minus(Y2, Y1), 2), zero=True)
        X3 = self._reduce(cs, self._minus(self._minus(self._product(cs, lam, lam), X1), X2))
        Y3 = self._reduce(cs, self._minus(self._product(cs, lam, self._minus(X1, X3)), Y1))
        return X3, Y3

    def _value(self, limbs):
        return limbs_int([v for _, v, _ in limbs], self.n)

    def hints(self, m0=2):
        """_PartialModDiv.hints with the multiply-divide records, whose cN and cD are literals like n"""
        if not getattr(self, "_declared", None):
            self.generate_constraints(_ValuesOnly(_LAYOUT_R))
        return [{key: v if key in ("op", "n", "literal", "cN", "cD") else [m0 + j for j in v] for key, v in hint.items()} for hint in self._declared]


class LimbModMulDiv(_PartialModMulDiv):
    """Non-native multiply-divide (the slope of a doubling, a modular multiply-add): per case (A, B, N+, N-, D+, D-) of integers their
    given limbs -- B = None: B is A, on the same columns; (N+, N-) or (D+, D-) = (None, None): no addend, no denominator (D = 1) --,
    Z from a multiply-divide hint with the literals cN and cD, and ONE exact check
        cD Z (D+ - D- + pad) - cN (A B + N+ - N- + pad) + product_pad = 0  (mod modulus)
    the products' blocks, then _reduce with a remainder that must be zero.  One ordinary row per case sums Z's limbs, and the public
    input is the sum of those.  operand_bits as in LimbModDiv."""

    def __init__(self, cases, modulus, n, limbs, cN=1, cD=1, decompose=True, operand_bits=None):
        self.cases, self.modulus, self.n, self.limbs, self.cN, self.cD = [tuple(c) for c in cases], int(modulus), n, limbs, int(cN), int(cD)
        self.decompose, self.operand_bits = decompose, operand_bits

    def generate_constraints(self, cs):
        self._setup(cs)
        sums = []
        given = lambda v: [] if v is None else self._given_limbs(cs, v, self.operand_bits)
        for A_v, B_v, Np_v, Nm_v, Dp_v, Dm_v in self.cases:
            assert (Np_v is None) == (Nm_v is None) and (Dp_v is None) == (Dm_v is None), "a pair of lists is absent as a pair"
            A = given(A_v)
            B = A if B_v is None else given(B_v)
            Np, Nm, Dp, Dm = given(Np_v), given(Nm_v), given(Dp_v), given(Dm_v)
            Z = self._muldiv(cs, A, B, Np, Nm, Dp, Dm, self.cN, self.cD)
            self._muldiv_check(cs, Z, A, B, Np, Nm, Dp, Dm, self.cN, self.cD)
            sums.append(Z)
        self._close(cs, sums)


def modmuldiv_cases(modulus, count, seed=SPLITMIX_SEED, cD=1, addend=True, denominator=True, square=False, narrow=None):
    """`count` cases (A, B, N+, N-, D+, D-) of integers for LimbModMulDiv, drawn from SplitMix64(seed); without `addend` or
    `denominator` that pair is (None, None), with `square` B is None (A's columns).  Operands as in moddiv_cases; a denominator for
    which cD (D+ - D-) has no inverse modulo a composite modulus is drawn again."""
    from math import gcd
    g = SplitMix64(seed)
    rnd = lambda bits: sum(g.next_u64() << (64 * i) for i in range(-(-bits // 64))) & ((1 << bits) - 1)
    draw = (lambda: rnd(modulus.bit_length() + 64) % modulus) if narrow is None else (lambda: sum(rnd(narrow[2]) << (narrow[0] * j) for j in range(narrow[1])))
    out = []
    while len(out) < count:
        A, B, Np, Nm, Dp, Dm = (draw() for _ in range(6))
        if gcd(cD * ((Dp - Dm) if denominator else 1) % modulus, modulus) == 1:
            out.append((A, None if square else B) + ((Np, Nm) if addend else (None, None)) + ((Dp, Dm) if denominator else (None, None)))
    return out


class EcDoubleAddChain(_PartialModMulDiv):
    """`steps` times R <- 2 R + Q on a short Weierstrass curve y^2 = x^3 + b over `modulus` (a = 0), on l limbs of n bits: R_0 =
    `point` and Q = `addend` are given.  Per step the tangent (_double: the slope 3 X^2 / (2 Y) is ONE multiply-divide hint, checked
    by lambda 2 Y - 3 X X = 0) and then the chord as in EcAddChain (_add).  One ordinary row per step sums the limbs of the new R;
    the public input is the sum of those.  The result is compared with affine arithmetic on Python integers; a vertical tangent or
    meeting x-coordinates is asserted."""

    def __init__(self, point, addend, modulus, n, limbs, steps, decompose=True):
        self.point, self.addend, self.modulus, self.n, self.limbs, self.steps = tuple(point), tuple(addend), int(modulus), n, limbs, steps
        self.decompose, self.operand_bits = decompose, None

    def result(self):
        """R_0 after `steps` times 2 R + Q, by the affine formulas on Python integers"""
        p, R = self.modulus, self.point
        for _ in range(self.steps):
            assert R[1] % p, "a vertical tangent: the doubling's slope is not defined"
            R = affine_add(p, R, R)
            assert (R[0] - self.addend[0]) % p, "the x-coordinates meet: the chord's slope is not defined"
            R = affine_add(p, R, self.addend)
        return R

    def generate_constraints(self, cs):
        self._setup(cs)
        want = self.result()         # asserts that every tangent and chord has a slope
        X1, Y1 = self._given_limbs(cs, self.point[0]), self._given_limbs(cs, self.point[1])
        X2, Y2 = self._given_limbs(cs, self.addend[0]), self._given_limbs(cs, self.addend[1])
        sums = []
        for _ in range(self.steps):
            X1, Y1 = self._double(cs, X1, Y1)
            X1, Y1 = self._add(cs, X1, Y1, X2, Y2)
            sums.append(X1 + Y1)
        assert (self._value(X1), self._value(Y1)) == want
        self._close(cs, sums)


# y^2 = x^3 + b as (p, b, order, G), and the literal point the verifier's accumulator starts from
SECP256K1 = (2 ** 256 - 2 ** 32 - 977, 7, 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141,
             (0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798, 0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8))
SECP256K1_START = (1004, 0x6FCBC4426CE7C7F6851B83EA89CD3F118ACFA8089CE3820ED5F2DEAB371701D4)
TOY_CURVE = (2 ** 22 - 3, 2, 4193929, (1, 2048))       # order prime, order < p < 2 order: the tests' curve, 22 scalar bits at (n, limbs) = (11, 2)
TOY_START = (1000, 1163942)


def ecdsa_schedule(curve, start, Q, u1, u2, bits):
    """The verifier's schedule on Python integers: acc = S; per bit from the top acc <- 2 acc, T = acc + G, acc <- b1 ? T : acc,
    T = acc + Q, acc <- b2 ? T : acc; then acc + (-[2^bits] S) = [u1] G + [u2] Q.  Both additions of a round are computed whatever the
    bits are, as the circuit computes them.  -> the result, or None where a step meets an exceptional case (a vertical tangent, meeting
    x-coordinates, the point at infinity)"""
    p, _, _, G = curve
    acc = start
    for i in reversed(range(bits)):
        if acc[1] % p == 0:
            return None
        acc = affine_add(p, acc, acc)
        for point, u in ((G, u1), (Q, u2)):
            if (acc[0] - point[0]) % p == 0:
                return None
            T = affine_add(p, acc, point)
            acc = T if (u >> i) & 1 else acc
    correction = affine_mul(p, 1 << bits, start)
    correction = (correction[0], -correction[1] % p)
    if (acc[0] - correction[0]) % p == 0:
        return None
    return affine_add(p, acc, correction)


def ecdsa_cases(curve, count, seed=SPLITMIX_SEED, start=None, bits=None):
    """`count` signatures (Q, h, r, s) for EcdsaVerify: key, nonce and hash from SplitMix64(seed), signing on Python integers.  A draw
    with r = 0, s = 0 or on which the verifier's schedule meets an exceptional case is drawn again."""
    p, _, order, G = curve
    start = start or (TOY_START if curve == TOY_CURVE else SECP256K1_START)
    bits = bits or order.bit_length()
    g = SplitMix64(seed)
    draw = lambda: sum(g.next_u64() << (64 * i) for i in range(-(-order.bit_length() // 64) + 1)) % (order - 1) + 1
    out = []
    while len(out) < count:
        d, k, h = draw(), draw(), draw()
        Q, R = affine_mul(p, d, G), affine_mul(p, k, G)
        r = R[0] % order
        s = pow(k, -1, order) * (h + r * d) % order
        if r == 0 or s == 0:
            continue
        w = pow(s, -1, order)
        got = ecdsa_schedule(curve, start, Q, h * w % order, r * w % order, bits)
        if got is None:
            continue
        assert got[0] % order == r
        out.append((Q, h, r, s))
    return out


class EcdsaVerify(_PartialModMulDiv):
    """ECDSA verification on y^2 = x^3 + b, `curve` = (p, b, order, G), on l limbs of n bits (order < 2^(n l)).  Given: the limbs of
    h, r, s, Qx, Qy.
        u1 = h / s, u2 = r / s mod order      modular hints (opcode 3) with their exact checks; their limbs are decomposed, and the
                                              bits are the selectors
        acc = S, a literal point; G           columns pinned by ordinary rows
        per bit from the top                  acc <- 2 acc (the slope a multiply-divide hint); T = acc + G; acc <- b1 ? T : acc by rows
                                              (T_j - acc_j) b1 = new_j - acc_j; the same with Q and b2
        R = acc + (-[2^bits] S)               the correction is computed here, on Python integers, and pinned like S
        R.x = q order + rem                   a long-division hint with _reduce's rows for the order
        rem_j - r_j = 0                       l check rows: the last rows of the system, and the only ones a wrong s fails
    One ordinary row sums rem's limbs into the public input.  The generator asserts that no step meets an exceptional case."""

    def __init__(self, curve, Q, h, r, s, n, limbs, start=None, decompose=True):
        self.curve, self.Q, self.h, self.r_sig, self.s, self.n, self.limbs = tuple(curve), tuple(Q), int(h), int(r), int(s), n, limbs
        self.start = tuple(start) if start else TOY_START if self.curve == TOY_CURVE else SECP256K1_START
        self.modulus, self.decompose, self.operand_bits = self.curve[0], decompose, None
        self.bits = n * limbs
        assert self.curve[2] < 1 << self.bits

    def _literal_point(self, cs, point):
        one = ConstraintSystem.ONE
        out = []
        for coordinate in point:
            limbs = []
            for v in int_limbs(coordinate, self.n, self.limbs):
                var = cs.new_witness_variable(v)
                cs.enforce_constraint([(v, one)], [(1, one)], [(1, var)])
                limbs.append(([(1, var)], v, (1 << self.n) - 1))
            out.append(limbs)
        return out

    def _select(self, cs, bit, bit_v, T, acc):
        """new_j = bit ? T_j : acc_j, by  (T_j - acc_j) bit = new_j - acc_j : one unknown, in C"""
        out = []
        for (lc_t, v_t, _), (lc_a, v_a, _) in zip(T, acc):
            v = v_t if bit_v else v_a
            var = cs.new_witness_variable(v)
            cs.enforce_constraint(_merged(lc_t + [(-c, x) for c, x in lc_a]), [(1, bit)], _merged([(1, var)] + [(-c, x) for c, x in lc_a]))
            out.append(([(1, var)], v, (1 << self.n) - 1))
        return out

    def generate_constraints(self, cs):
        self._setup(cs)
        one, n = ConstraintSystem.ONE, self.n
        p, _, order, G = self.curve
        h, r_sig, s = (self._given_limbs(cs, v) for v in (self.h, self.r_sig, self.s))
        Qx, Qy = self._given_limbs(cs, self.Q[0]), self._given_limbs(cs, self.Q[1])
        scalars = []
        with self._over(order):
            decompose, self.decompose = self.decompose, False
            for numerator in (h, r_sig):
                u = self._quotient(cs, numerator, [], s, [])          # raises where s has no inverse: s = 0
                self._reduce(cs, self._minus(self._product(cs, u, s), numerator), zero=True)
                scalars.append(u)
            self.decompose = decompose
        selectors = []
        for u in scalars:
            bits = []
            for lc, v, _ in u:
                limb_bits = _new_bits(cs, v, n)
                cs.enforce_constraint(lc, [(1, one)], _weighted(limb_bits))
                bits += [(b, (v >> i) & 1) for i, b in enumerate(limb_bits)]
            selectors.append(bits)
        u1, u2 = self._value(scalars[0]), self._value(scalars[1])
        want = ecdsa_schedule(self.curve, self.start, self.Q, u1, u2, self.bits)
        assert want is not None, "a step of the schedule meets an exceptional case"
        acc = self._literal_point(cs, self.start)
        Gl = self._literal_point(cs, G)
        correction = affine_mul(p, 1 << self.bits, self.start)
        for i in reversed(range(self.bits)):
            acc = self._double(cs, *acc)
            for point, bits in ((Gl, selectors[0]), ((Qx, Qy), selectors[1])):
                T = self._add(cs, acc[0], acc[1], point[0], point[1])
                bit, bit_v = bits[i]
                acc = [self._select(cs, bit, bit_v, T[k], acc[k]) for k in range(2)]
        Rx, Ry = self._add(cs, acc[0], acc[1], *self._literal_point(cs, (correction[0], -correction[1] % p)))
        assert (self._value(Rx), self._value(Ry)) == want
        with self._over(order):
            rem = self._reduce(cs, Rx)
        self._close(cs, [rem])
        for (lc, _, _), (lc_r, _, _) in zip(rem, r_sig):
            cs.enforce_constraint(lc + [(-c, x) for c, x in lc_r], [(1, one)], [])

    def accepts(self):
        """whether R.x mod order = r on Python integers (the last rows hold)"""
        order = self.curve[2]
        w = pow(self.s, -1, order)
        R = ecdsa_schedule(self.curve, self.start, self.Q, self.h * w % order, self.r_sig * w % order, self.bits)
        return R is not None and R[0] % order == self.r_sig


def _invertible(rows, r):
    """whether the square matrix `rows` is invertible mod r: elimination on Python integers"""
    rows = [list(row) for row in rows]
    for c in range(len(rows)):
        pivot = next((i for i in range(c, len(rows)) if rows[i][c]), None)
        if pivot is None:
            return False
        rows[c], rows[pivot] = rows[pivot], rows[c]
        inv = pow(rows[c][c], r - 2, r)
        for i in range(c + 1, len(rows)):
            f = rows[i][c] * inv % r
            if f:
                rows[i] = [(v - f * w) % r for v, w in zip(rows[i], rows[c])]
    return True


class LinearBlocks(_Partial):
    """`count` square linear systems, each with a random m x m matrix M mod r of its own (drawn from SplitMix64(seed), redrawn while
    singular; the assignment's values come from SplitMix64(values), so that one key serves many assignments): per system the given witnesses g_i and h_i, the witnesses u_j and the rows  (g_i + h_i) * 1 = sum_j M_ij u_j , then
    (sum u_j) * 1 = s ; the public input is sum s.  The u_j and h_i are drawn and g_i = sum_j M_ij u_j - h_i, so the assignment comes
    from Python integers without an inversion.  One dependency level of `count` linear blocks with `count` distinct matrices."""

    _matrices = {}   # (r, m, count, seed) -> the matrices: part of the key, drawn and tested once

    def __init__(self, m, count, seed=SPLITMIX_SEED, values=None):
        assert m >= 2 and count >= 1
        self.m, self.count, self.seed, self.values = m, count, seed, seed + 1 if values is None else values

    def matrices(self, r):
        key = (r, self.m, self.count, self.seed)
        if key not in self._matrices:
            gen, m, mats = SplitMix64(self.seed), self.m, []
            while len(mats) < self.count:
                mat = [[gen.fr(r) for _ in range(m)] for _ in range(m)]
                if _invertible(mat, r):
                    mats.append(mat)
            self._matrices[key] = mats
        return self._matrices[key]

    def _systems(self, r):
        """-> per system (M, g, h, u) on Python integers; u and h are drawn from SplitMix64(values)"""
        gen, m, out = SplitMix64(self.values), self.m, []
        for mat in self.matrices(r):
            u, h = [gen.fr(r) for _ in range(m)], [gen.fr(r) for _ in range(m)]
            g = [(sum(c * v for c, v in zip(row, u)) - h_i) % r for row, h_i in zip(mat, h)]
            out.append((mat, g, h, u))
        return out

    def generate_constraints(self, cs):
        self._chosen = []
        one, r = ConstraintSystem.ONE, cs.r
        total, total_v = [], 0
        for mat, g_v, h_v, u_v in self._systems(r):
            g = [self._given(cs, v) for v in g_v]
            h = [self._given(cs, v) for v in h_v]
            u = [cs.new_witness_variable(v) for v in u_v]
            for i, row in enumerate(mat):
                cs.enforce_constraint([(1, g[i]), (1, h[i])], [(1, one)], [(c, v) for c, v in zip(row, u) if c])
            s = cs.new_witness_variable(sum(u_v))
            cs.enforce_constraint([(1, v) for v in u], [(1, one)], [(1, s)])
            total.append((1, s))
            total_v += sum(u_v)
        out = cs.new_input_variable(total_v)
        cs.enforce_constraint(total, [(1, one)], [(1, out)])

    def native(self, r):
        """-> (instance, witness) on Python integers, without generating a row: per system g, h, u and sum u"""
        witness, total = [], 0
        for _, g, h, u in self._systems(r):
            witness += g + h + u + [sum(u) % r]
            total += sum(u)
        return [1, total % r], witness


def row_order(nr, order, blocks=1):
    """The row order Reordered replays: a permutation of range(nr).  `order` is "reverse", an int (the seed of a Fisher-Yates shuffle
    on SplitMix64) or an explicit permutation; with blocks = k it moves whole k-row blocks (the last one may be shorter) and an
    explicit permutation is one of the block indices -- rows keep their order inside a block."""
    n_blocks = -(-nr // blocks)
    if isinstance(order, str):
        if order != "reverse":
            raise ValueError("order is 'reverse', a seed or a permutation")
        perm = list(range(n_blocks))[::-1]
    elif isinstance(order, int):
        g, perm = SplitMix64(order), list(range(n_blocks))
        for i in range(n_blocks - 1, 0, -1):
            j = g.next_u64() % (i + 1)
            perm[i], perm[j] = perm[j], perm[i]
    else:
        perm = list(order)
        if sorted(perm) != list(range(n_blocks)):
            raise ValueError("order is no permutation of the %d blocks" % n_blocks)
    return [row for blk in perm for row in range(blk * blocks, min((blk + 1) * blocks, nr))]


class Reordered:
    """`circuit` with its constraint rows emitted in another order (row_order): the same variables, allocated in the inner circuit's
    order, the same rows, the same assignment -- what an R1CS assembled from parts, a row-sorted matrix file or a producer that emits
    assertions first looks like.  The inner circuit is generated into a private ConstraintSystem and its enforce_constraint calls
    are replayed in the new order.  partial() and native() are the inner circuit's.  With blocks = k whole k-row gadgets move, so that
    an is-zero pair's opener stays before its closer (a closer examined first is an ordinary dividing step)."""

    def __init__(self, circuit, order, blocks=1):
        self.circuit, self.order, self.blocks = circuit, order, blocks

    def generate_constraints(self, cs):
        inner = ConstraintSystem(cs.r)
        self.circuit.generate_constraints(inner)
        var = {ConstraintSystem.ONE: ConstraintSystem.ONE}
        for i, value in enumerate(inner.instance[1:], 1):
            var[("inst", i)] = cs.new_input_variable(value)
        for i, value in enumerate(inner.witness):
            var[("wit", i)] = cs.new_witness_variable(value)
        for row in row_order(len(inner.rows), self.order, self.blocks):
            cs.enforce_constraint(*([(coef, var[v]) for coef, v in lc] for lc in inner.rows[row]))

    def partial(self, *args, **kwargs):
        return self.circuit.partial(*args, **kwargs)

    def native(self, *args, **kwargs):
        return self.circuit.native(*args, **kwargs)


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
