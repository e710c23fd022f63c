// Witness solving, host side: the PLAN that completes a partial assignment by forward propagation through the rows of an R1CS
// (DESIGN.md §4.10).  Header-only, no HIP: the library's driver (csrc/solve.hip, through csrc/solve_steps.cuh) and six CPU programs
// (tests/native/solve_plan_selftest.cpp, solve_bits_selftest.cpp, solve_iszero_selftest.cpp, solve_order_selftest.cpp,
// solve_divrem_selftest.cpp, solve_indicator_selftest.cpp, through their rig tests/native/solve_selftest.hpp) include the same file.
// (A seventh program on the same rig, solve_sqrt_selftest.cpp, pins the square-root row below, an eighth, solve_block_selftest.cpp,
// the scheduler's linear blocks.)
//
// Input: the three matrices in CSR form with the first-entry rule already applied (a column occurs at most once per row and
// matrix: the key's resident matrices are like that), m0 + mw columns and one byte per column, non-zero = unknown (1: unknown;
// 2: unknown, and a Euclidean quotient -- the caller's second marker, which has meaning in a division row only; 3: unknown, and
// the indicator of its guard row -- the third marker, which has meaning in an indicator row only; 4: unknown, and the smaller square
// root of its square-root row -- the fourth marker, which has meaning in a square-root row only).  A stored entry
// whose coefficient is zero names no variable.  Rows are visited ONCE, in matrix order; at row r, with the columns solved so far:
//   no unknown column                         a check row, skipped
//   one unknown u, in exactly one of A, B, C  a solve step (kind = the matrix that holds u); u is known from here on
//   anything else                             the structure is unsolvable: the error names the row
// and a marked column that no row determines is an error that names the column.
//
// With the field's modulus (four 64-bit words; the coefficients are canonical Montgomery words) two more rows are understood, so
// that bit decompositions -- and with them boolean circuits -- complete:
//   booleanity    the only unknown is u, C_r has no non-zero entry, and {A_r, B_r} = {k z_u, k' (1 - z_u)}: one side is the single
//                 entry (k, u), the other exactly the two entries (k', column 0) and (-k', u), k and k' non-zero.  The row marks u
//                 BOOLEAN-PENDING, remembers r and is otherwise a check row.  One unknown in two matrices in any other shape is
//                 ERR_TWO_MATRICES at once.
//   decomposition k >= 2 unknowns, all boolean-pending, all in the same one of A, B, C and in no other, with coefficients
//                 c 2^0 ... c 2^(k-1), each exactly once in any stored order, c non-zero, k <= bitlength(r) - 1 (the solution is then
//                 unique).  ONE step (kind BITS_C / BITS_A / BITS_B) that determines all k columns: t as for the ordinary kinds with
//                 the k entries left out and coef = c; z_{u_i} = bit i of the canonical integer of t.  t >= 2^k is stuck at run time.
//                 Step::pos / col name the entry that holds c, Plan::bit_cols[cols_off .. cols_off + bits) the columns in exponent
//                 order.  Any other row with two or more unknowns is ERR_MANY_UNKNOWNS; the message says which condition failed.
//                 Booleanity rows that come AFTER the decomposition row are not looked for: that decomposition row is refused.
// A boolean-pending column that is the single unknown of a later ordinary row is solved by it.  One still pending at the end of the
// pass is ERR_TWO_MATRICES naming its booleanity row (the smallest such row), before ERR_UNDETERMINED is looked for.
//   is-zero pair  two rows with two fresh unknowns m (the multiplier) and b (the flag), the shape every equality test compiles to:
//                 arkworks  (a - b) mult = neq ; (a - b) (1 - neq) = 0     circom IsZero  (-in) inv = out - 1 ; in out = 0
//                 OPENER r1: exactly two distinct unknowns, each named once.  One of A_r1, B_r1 is the known side K1 (no unknown, at
//                 least one non-zero entry), the other has (cm, m) as its only non-zero entry; C_r1 names b with coefficient cb
//                 beside any known rest.  Both columns become PAIR-PENDING and the row is otherwise skipped; any number of openers
//                 may be pending.  CLOSER r2: the first later row that names m or b.  It names b and not m, b is its only unknown,
//                 in exactly one of A_r2, B_r2 (coefficient kb beside any known rest) and not in C_r2; the other of A_r2, B_r2 is
//                 K2 = K1 or -K1 as a linear combination: the same non-zero (column, coefficient) entries in any stored order, or
//                 every coefficient negated (a + a' = 0 by add_mod: no field multiplication here).  The pair is ONE step of kind
//                 KIND_ISZERO at row r2 that determines both columns; with d = K1 z:
//                     d != 0:  b = ((C_r2 z) / (K2 z) - rest_r2) / kb,  m = ((C_r1 z, with b) / d) / cm
//                     d == 0:  b = -C_r1_rest / cb,                     m = 0      (m is free then: circom's convention, and 0^(r-2))
//                 The step never sticks.  A caller that wants another m supplies it: only b is unknown then and r1 is an ordinary
//                 kind-C step.  Step::pos / col name b's entry in the closer, Plan::pairs[cols_off] carries the rest (a side list, as
//                 bit_cols is: the step record of the other kinds is what it was).  A two-unknown row that is no opener is refused at once, as before; a pair that does not close is
//                 ERR_MANY_UNKNOWNS at r1 with the message the row has without the modulus, then what failed.  Openers pending
//                 when the rows end are reported first, smallest r1 first.
//   division row  ONE row with two fresh unknowns q (the quotient) and rem (the remainder), each named once: circom's
//                 q <-- a \ b; r <-- a % b; q*b + r === a, arkworks' DIV / REM and reductions by a non-power-of-two modulus.  One of
//                 A_r, B_r has (cq, q) as its only non-zero entry and q carries pattern byte 2 (the caller says "a quotient": the
//                 shape is the opener's, and nothing is guessed); the other is the known divisor side K (no unknown, at least one
//                 non-zero entry); C_r names rem with coefficient cr = -cq (a + a' = 0 by add_mod) beside any known rest R.  ONE step
//                 of kind KIND_DIVREM at row r that determines both columns, at 1 + max level of what the row reads; with d = K z and
//                 a = R / cq as canonical integers:
//                     d != 0:  q = floor(a / d),  rem = a mod d      (both below r; q d + rem = a in the integers, so the row holds)
//                     d == 0:  stuck at row r, zero in both columns
//                 Step::pos / col name q's entry, Plan::divs[cols_off] carries rem's entry in C and which side K is.  Such a row is a
//                 division step at once: it is never registered as an opener and never waits for a closer.  Byte 2 has meaning in
//                 that position only: a byte-2 column that is the single unknown of an ordinary row is solved by that row, and one
//                 named anywhere else behaves as a plain unknown.  A row with two or more unknowns whose byte-2 column is the lone
//                 entry of A or B and which misses a condition is ERR_MANY_UNKNOWNS at once, with the message the row had before and
//                 ", and no division row: " + the condition: cr != -cq; rem in A or B; rem named twice; the other side not known
//                 (an unknown on it, or no non-zero entry); the quotient named twice; a third unknown.  In the scheduler below such
//                 a row WAITS instead, and is a division step as soon as q and rem are its only unknowns.
//                 Not handled: signed division, cr != -cq, a known rest beside q on its side, a division without the marker.
//   indicator row ONE row whose only unknown u carries pattern byte 3 (the caller's third marker: "the indicator of its guard row")
//                 and is named exactly once, as the ONLY non-zero entry (k, u) of A_r or B_r; the other of the two is the known guard
//                 side K (no unknown, at least one non-zero entry) and C_r has no non-zero entry: circomlib's Decoder / Multiplexer,
//                 out[i] <-- (inp == i) ? 1 : 0;  out[i] * (inp - i) === 0.  ONE step of kind KIND_INDICATOR at 1 + max level of what K
//                 reads:  z_u = (K z == 0) ? 1 : 0, as field one or field zero whatever k is.  The step never divides, needs no inverse
//                 and never leaves an assignment stuck.  The rows do not determine the value at the hit (0 satisfies them too): it is a
//                 hint, and the marker says so; with the plain marker the row is the ordinary dividing step it always was, which is
//                 stuck at the hit.  Step::pos / col name u's entry, Step::cols_off says which side it lies on.  The rule applies
//                 wherever a row's single unknown, named once, makes an ordinary step (here, and in the scheduler below its one-unknown
//                 and released-multiplier cases).  Byte 3 has meaning in that position only: a byte-3 column that is the single unknown
//                 of a row of any other shape (C_r not empty, other non-zero entries beside u on its side, an empty other side) is solved
//                 by that row as an ordinary step, and named beside other unknowns it is a plain unknown.  No refusal is added.
//                 Not handled: a hit value other than 1, a non-empty C_r, a known rest beside u, inferring indicators without the
//                 marker, sharded keys, per-assignment patterns.
//   square-root row  ONE row whose only unknown u carries pattern byte 4 (the caller's fourth marker: "the square root of its row") and is
//                 named exactly twice: as the ONLY non-zero entry (ka, u) of A_r and as the ONLY non-zero entry (kb, u) of B_r; C_r names
//                 no unknown and does not name u, and may be empty: circom's  x <-- sqrt(u); x*x === u  (circomlib's pointbits.circom,
//                 Bits2Point_Strict) and arkworks' sqrt witness in point decompression.  ONE step of kind KIND_SQRT at 1 + max level of
//                 what C_r reads; with c = (C z)_r / (ka kb):
//                     c a square, 0 included:  z_u = the root whose canonical integer is the smaller of the pair, <= (r - 1) / 2 (what
//                                              circom's sqrt returns)
//                     c a non-residue:         stuck at row r, zero stored (the handling of a zero divisor: the stuck word is lowered
//                                              through the sink, and the root-cause rule applies under a reordered plan)
//                 The rows do not determine the value (-u satisfies them too): it is a hint, and the marker says so.  Step::pos / col
//                 name u's entry in A_r, Step::cols_off is the offset of u's entry in B_r from the start of that row; the step's
//                 inverse is 1 / (ka kb), and a launch that holds such a step is a dividing one.  Byte 4 has meaning in that position
//                 only: a byte-4 column that is the single unknown of an ordinary row, named once, is solved by that row, and named
//                 beside other unknowns it is a plain unknown.  With the plain marker on u the row plans, waits and is refused exactly
//                 as before (u u = ... : ERR_TWO_MATRICES in matrix order; in any order it waits for a row that determines u): no
//                 plan, message or word changes and no refusal is added.  In the scheduler below such a row waits on the unknowns of
//                 C_r like any other row and acts when u is the only one left; an opener registered over u (the row x = u * s has that
//                 shape) was none: it is RELEASED and examined again.
//                 Not handled: a known rest beside u on either side ((u + k)(u + k) = c), u in C_r (a general quadratic),
//                 the larger root or arkworks' unspecified choice of root (a caller who wants either supplies u itself),
//                 inferring a square root without the marker, sharded keys, per-assignment patterns.
// Without the modulus (nullptr) all five additions are off.  (So is the sixth, the square-root row.)  (And the linear blocks: they are the scheduler's, which runs with the modulus only.)
//
// build_plan_any_order drops the matrix order: it runs build_plan, and where that refuses, a WAITING-ROW SCHEDULER examines the rows
// from a min-heap (at first all of them) against the same column state with the same rules, except that these refusals become waiting:
//   no unknown                              a check row
//   only the flag b of a registered opener  the closer (b once, in A or B, not in C, the other side +-K1): the KIND_ISZERO step, at
//                                           1 + max of what both rows read.  Any other shape is a DEFINITE refusal, as in matrix order
//   only the multiplier m of one, once      an ordinary step that determines m; the opener was none: it is RELEASED and examined again
//   a division row, q and rem its only      the KIND_DIVREM step at once; an opener registered over q or rem (rem * 1 = y has that shape)
//   unknowns                                was none: it is RELEASED and examined again
//   a pair-pending column in any other way  the row WAITS (the multiplier beside something else, a second unknown, an opener-shaped
//                                           row over a pending column)
//   one unknown, named once                 an ordinary step, or -- byte 3 on it and the indicator shape -- the KIND_INDICATOR step
//   one unknown, byte 4, named twice, as    the KIND_SQRT step at once; an opener registered over u was none: it is RELEASED and examined
//   the lone entries of A_r and of B_r      again
//   one unknown, named several times        booleanity: boolean-pending; any other shape WAITS (a later row may determine the column
//                                           and this one is a check row then)
//   two or more unknowns                    a decomposition: the bits step; a division row: its step; the opener shape without the
//                                           quotient's marker on the lone entry: registered; anything else WAITS
//   two or more unknowns, all in C_r only,  a LINEAR ROW over the set S of its unknown columns: parked like any waiting row, and
//   none boolean- or pair-pending           registered under the sorted S (below)
// A waiting row is parked on its unknown columns and returns to the heap when one of them becomes known, boolean-pending or released.
//   linear block  k = |S| >= 2 rows whose unknowns are the SAME k columns, each named in C_r only (A_r and B_r name no unknown; either
//                 may be empty, the product is then 0), none of them boolean- or pair-pending, and which no rule above claims: the
//                 shape of non-native multiplication (ark-r1cs-std's mul_without_reduce, circom-bigint's BigMultNoCarry), which pins
//                 the 2l - 1 limbs p_j of a product by  (sum a_i c^i) (sum b_i c^i) = sum p_j c^j  at 2l - 1 points c.  No row order
//                 propagates through such rows, but together they are a square linear system whose matrix is part of the key.  When
//                 the k-th linear row with exactly the set S is registered and k <= 64, those k rows and k columns become ONE step of
//                 kind KIND_BLOCK at 1 + max level of every column the k rows read; all k columns get that level, and later rows over
//                 S are check rows.  A column of S that becomes known by another route wakes the row, which is examined again with
//                 its smaller set (a c = 0 row a_0 b_0 = p_0 is an ordinary step, and the others a block over 2l - 2 columns).
//                 Plan::blocks[cols_off] carries the rows and columns, both ascending, and an index into Plan::block_mats, the
//                 DISTINCT matrices M[i][j] = the coefficient of S_j in C_{r_i} (zero where absent), compared word for word: the
//                 planner multiplies nothing, and 10 000 products at the same points share one Vandermonde matrix.  The driver
//                 inverts each distinct matrix once per plan (solve_steps.cuh: solve_block_invert) and refuses a singular one; the
//                 step is then  z_S = M^-1 (A z B z - C_known z)  over the k rows: no division, never stuck.  Step::row / col name
//                 the smallest row and column, Step::pos is not used.  A block step is a launch of its own (LAUNCH_BLOCK), whatever
//                 the level's width.  Pattern bytes 2, 3 and 4 on a column of S have no meaning there.  The rule is the scheduler's:
//                 build_plan refuses the first such row as it always did.  A set of more than 64 columns keeps waiting, and the
//                 refusal then ends ", and no linear block: k unknowns exceed 64"; fewer than k linear rows for a set is the refusal
//                 it always was.
//                 Not handled: an unknown in A_r or B_r (the matrix would depend on the assignment), rows over different sets
//                 (banded or triangular systems), k > 64, boolean- or pair-pending columns in S, choosing an independent subset when
//                 the first k rows are dependent, sharded keys, per-assignment patterns.
//   declared hint a LONG DIVISION that the key declares (pm_pk_set_hints; decode_hints below), not a row shape: kq quotient columns, kr
//                 remainder columns, kD dividend columns and kE divisor columns (or kE literal limbs), limbs of n bits.  Every such
//                 gadget -- circom-bigint's BigMod / BigMultModP (div[i] <-- long_div(..)), ark-r1cs-std's non-native reduce --
//                 witnesses q and rem as multi-word integers that no row determines: the limb equations are underdetermined and
//                 uniqueness comes from the range checks, so there is no shape to recognise.  A hint is ACTIVE in a call when all its
//                 outputs carry the plain unknown marker (byte 1), INERT when all are given (the caller supplied q and rem: nothing
//                 changes), and refused when some are marked and some given or one carries byte 2, 3 or 4.  With an active hint the
//                 system goes to the scheduler only.  An output column of an active hint is HINT-OWNED: no row solves it, and a row
//                 that names one while it is unknown waits (it is a check row, or an ordinary row over its other unknown, once the
//                 hint has acted).  A hint waits on its unknown input columns like a row and acts when none is left: ONE step of kind
//                 KIND_LONGDIV at 1 + max level of its inputs; all kq + kr outputs get that level and wake their waiters.  With
//                 D = sum_j int(z_{D_j}) 2^(n j) and E = sum_j int(z_{E_j}) 2^(n j) (int: the canonical integer; limbs need not be
//                 normalised -- the overflowing limbs of a no-carry product are the intended dividend) the step stores the kq n-bit
//                 limbs of floor(D / E) and the kr n-bit limbs of D mod E.  Stuck, with zero in every output: E = 0, D >= 2^1024,
//                 E >= 2^512, q >= 2^(n kq), rem >= 2^(n kr).  Step::row is nr + h for hint h of the declaration -- a value no row
//                 has, and the stuck word of the step; Step::col is its first quotient column, Step::cols_off its entry of
//                 Plan::hints.  Hint steps sort last within a level, after the blocks, and are a launch of their own
//                 (LAUNCH_LONGDIV, not dividing) whatever the level's width; Launch::rounds is the division's trip count for the launch, the
//                 largest min(1024, n (kD - 1) + 256) of its hints.  A hint that never becomes ready is refused as
//                 "hint h: input column c is never determined", followed by the scheduler's text for the first column that stays unknown.
//                 Not handled by the long-division record: other opcodes (modular inverse, gcd, sorting), signed limbs, dividends beyond 1024 bits (RSA-2048),
//                 hints on sharded keys, per-assignment declarations, inferring a hint from rows.  Of these, modular inverse and
//                 modular division now have a record of their own:
//   modular hint  a MODULAR DIVISION that the key declares in the same stream (opcode HINT_MODDIV = 3; 2 stays reserved and refused):
//                 kz output columns, kNp + kNm numerator columns, kDp + kDm denominator columns, kP modulus columns (or kP literal
//                 limbs), limbs of n bits.  The slope (Y2 - Y1) / (X2 - X1) of an affine point addition, ark-r1cs-std's non-native
//                 inverse, circom-ecdsa's BigModInv: the circuit checks Z D = N (mod P) through the product-and-reduce path, and no
//                 row determines Z.  ACTIVE / INERT / refused, HINT-OWNED outputs, waiting on inputs and the never-ready refusal are
//                 the long-division rules, applied to the kz outputs.  It acts as ONE step of kind KIND_MODDIV at 1 + max level of
//                 its inputs, Step::row = nr + h, Step::col its first output, Step::cols_off its entry of Plan::hints.  With each list
//                 the sum of int(z_{c_j}) 2^(n j) (limbs need not be normalised), N = N+ - N- (kNp = kNm = 0: N = 1, a plain
//                 inverse), D = D+ - D- and P the modulus, the step stores the kz n-bit limbs of the unique Z in [0, P) with
//                 Z D = N (mod P).  Stuck, with zero in every output: P even or P < 3, P >= 2^512, N+, N-, D+ or D- >= 2^1024,
//                 gcd(D mod P, P) != 1 (D = 0 mod P included; P need not be prime), Z >= 2^(n kz).  The modular hints of a level
//                 sort after its long divisions and are a launch of their own (LAUNCH_MODDIV) with
//                 two trip counts: Launch::rounds, the largest min(1024, n (k - 1) + 256) over the operand lists of its hints (the
//                 reductions modulo P), and Launch::inv_rounds = 2 L, L the largest min(512, n (kP - 1) + 256) (the inversion).
//                 Not handled: even moduli, operands beyond 1024 bits, the slope of a doubling as one hint (3 X^2 / 2 Y: the
//                 numerator is a product), gcd, sorting.  Of the long-division record's list, dividends beyond 1024 bits now
//                 have a record of their own:
//   wide hint     a WIDE LONG DIVISION that the key declares in the same stream (opcode HINT_LONGDIV_WIDE = 5; 2 and 4 stay refused as
//                 unknown): the record of opcode 1 -- n, kq, kr, kD, kE, flags, the four column lists or kE literal limbs -- with
//                 kD <= 128, kE <= 64, kq <= 128, kr <= 64, n (kD - 1) < 8192 and n (kE - 1) < 4096.  An RSA-2048 modular
//                 multiplication divides some 4200 bits by 2048: 32 limbs of 64 bits, or zk-email's 17 of 121.  ACTIVE / INERT /
//                 refused, HINT-OWNED outputs, waiting on inputs and the never-ready refusal are the long-division rules unchanged;
//                 all three opcodes share the index h and the set of output columns.  It acts as ONE step of kind KIND_LONGDIV_WIDE
//                 at 1 + max level of its inputs, Step::row = nr + h, Step::col its first quotient column, Step::cols_off its entry
//                 of Plan::hints, and stores the kq n-bit limbs of floor(D / E) and the kr n-bit limbs of D mod E.  Stuck, with zero
//                 in every output: E = 0, D >= 2^8192, E >= 2^4096, q >= 2^(n kq), rem >= 2^(n kr).  The wide hints of a level sort
//                 last, after its modular ones, and are a launch of their own (LAUNCH_LONGDIV_WIDE: a WAVE per hint,
//                 not a lane); Launch::rounds is the largest min(8192, n (kD - 1) + 256) of the range, a bound
//                 that sizes things -- the division's trip counts follow the operands (solve_steps.cuh: longdiv_wide_words).
//                 Opcode 1 is not widened: its limits, its kernel and its plans are what they were.
//                 Not handled: modular division at these widths (HINT_MODDIV keeps 1024 / 512 bits), even moduli, linear blocks
//                 beyond 64 unknowns (RSA-4096 at 64-bit limbs), hints on sharded keys, per-assignment declarations, gcd, sorting.
//                 Of the modular record's list, the slope of a doubling now has a record of its own:
//   multiply-divide hint  a MODULAR MULTIPLY-DIVIDE that the key declares in the same stream (opcode HINT_MODMULDIV = 7; 2, 4 and 6 stay
//                 refused as unknown, and so is 8): kz output columns, kA + kB factor columns, kNp + kNm addend columns, kDp + kDm
//                 denominator columns, kP modulus columns (or kP literal limbs), limbs of n bits, and two one-word literals cN and cD
//                 in 1 .. 2^32 - 1.  The slope 3 X^2 / (2 Y) of a tangent (circom-ecdsa's Secp256k1Double: A = B = X, D+ = Y, cN = 3,
//                 cD = 2), and with kDp = kDm = 0 (D = 1) a modular multiply-add, the remainder of A B + C without its quotient.
//                 ACTIVE / INERT / refused, HINT-OWNED outputs, waiting on inputs and the never-ready refusal are the long-division
//                 rules, applied to the kz outputs; all four opcodes share the index h and the set of output columns.  It acts as
//                 ONE step of kind KIND_MODMULDIV at 1 + max level of its inputs, Step::row = nr + h, Step::col its first output,
//                 Step::cols_off its entry of Plan::hints.  With each list the sum of int(z_{c_j}) 2^(n j) (limbs need not be
//                 normalised; A and B may name the same columns) the step stores the kz n-bit limbs of the unique Z in [0, P) with
//                 cD (D+ - D-) Z = cN (A B + N+ - N-)  (mod P).  Stuck, with zero in every output: P even or P < 3, P >= 2^512, any
//                 of the six list sums >= 2^1024, gcd(cD D mod P, P) != 1 (D = 0 mod P included, and a cD that shares a factor with a
//                 composite P), Z >= 2^(n kz) -- and nothing else: cN and cD scale AFTER the reductions, when the value is below P.
//                 The multiply-divide hints of a level sort last, after its wide ones, and are a launch of their own
//                 (LAUNCH_MODMULDIV, not dividing, never chained) with two trip counts: Launch::rounds, the largest
//                 min(1024, n (k - 1) + 256) over the six lists of its hints, and Launch::inv_rounds = 2 L, L the largest
//                 min(512, n (kP - 1) + 256) -- the inversion's trip count and, since the product of two residues is below 2^(2 L),
//                 the trip count of the product's reduction as well.  Opcode 3 is not touched: its record, its kernel and its plans
//                 are what they were.
//                 Not handled: curves with a != 0 need no more than N+ = a (the record allows it); complete addition formulas,
//                 windowed or GLV scalar multiplication, operands beyond 1024 bits, even moduli, hints on sharded keys,
//                 per-assignment declarations.
// With the heap empty the scheduler has failed if an opener is unclosed, a boolean-pending column unsolved or a marked column
// undetermined; the result is then build_plan's error (code, row, column, message) with "; in any row order: ..." appended.  A plan
// it finds has Plan::reordered = true, level(step) as below, the steps sorted by (level, kind, row) and the level_ptr and launches of
// the same tail (finish_plan).  O(nnz log rows); a reversed chain costs one examination and one wake-up per row, not a sweep per level.
// Unchanged by the any-order route:
//   - a closer examined BEFORE its opener is an ordinary dividing step, and the opener an ordinary kind-C step: it sticks at d = 0
//   - K2 = lambda K1 for another lambda than +-1 is not recognised
//   - a known rest beside m in the opener is not handled
//   - the bits of one decomposition over two matrices are not handled
//   - one pattern per batch: per-assignment patterns are not supported; nor are sharded keys
//
// level(step) = 1 + max level of the columns the row reads (given columns: level 0); a decomposition gives all its columns that
// level.  The steps come out sorted by level, inside a level by kind (C first: the kinds that divide share a launch; then the
// decompositions in the same order, then the is-zero pairs, then the division rows, then the indicator rows, then the square-root rows, then the linear blocks, then the declared hints, the multiply-divide ones last), stable by row -- one counting sort.  O(nnz + columns), plus k log k per decomposition.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <functional>
#include <map>
#include <queue>
#include <string>
#include <utility>
#include <vector>

namespace pmsolve {

// z_u = (Az Bz - C_rest) / coef;  (Cz / Bz - A_rest) / coef;  (Cz / Az - B_rest) / coef;  KIND_BITS_x = KIND_BITS_C + x: a decomposition
// KIND_ISZERO: an is-zero pair, both columns in one step;  KIND_DIVREM: a division row, quotient and remainder in one step
// KIND_INDICATOR: an indicator row, z_u = [K z == 0]: no division and no inverse
// KIND_SQRT: a square-root row, z_u = the smaller root of (C z)_r / (ka kb); its inverse is 1 / (ka kb), so it counts as dividing
// KIND_BLOCK: a linear block, z_S = M^-1 rhs over k rows and k columns; the inverse is plan data, so it does not count as dividing
// KIND_LONGDIV: a declared long-division hint, kq + kr columns in one step; integer arithmetic only, so it does not count as dividing
// KIND_MODDIV: a declared modular-division hint, kz columns in one step; integer arithmetic only as well
// KIND_LONGDIV_WIDE: a declared wide long division (opcode 5), kq + kr columns in one step of one wave; integer arithmetic only
// KIND_MODMULDIV: a declared modular multiply-divide (opcode 7), kz columns in one step; integer arithmetic only
enum Kind : uint32_t { KIND_C = 0, KIND_A = 1, KIND_B = 2, KIND_BITS_C = 3, KIND_BITS_A = 4, KIND_BITS_B = 5, KIND_ISZERO = 6, KIND_DIVREM = 7, KIND_INDICATOR = 8, KIND_SQRT = 9, KIND_BLOCK = 10, KIND_LONGDIV = 11, KIND_MODDIV = 12, KIND_LONGDIV_WIDE = 13, KIND_MODMULDIV = 14 };
constexpr uint32_t NUM_KINDS = 7;        // the kinds that need no second marker: what it always counted
constexpr uint32_t NUM_STEP_KINDS = 8;   // KIND_C .. KIND_DIVREM, the kinds whose value comes from field or integer arithmetic on the row: what it counted when kind 7 came
constexpr uint32_t NUM_SORT_KINDS = 10 + 1;  // all 11 of them: the ten kinds that one lane executes, KIND_INDICATOR and KIND_SQRT included, and KIND_BLOCK: the kinds that rows make
constexpr uint32_t NUM_PLAN_KINDS = 12;  // with KIND_LONGDIV, which no row makes: the key width of finish_plan's counting sort (NUM_SORT_KINDS counts the kinds that rows make, as it did)
constexpr uint32_t NUM_HINT_KINDS = 13;  // with KIND_MODDIV: the key width of finish_plan's counting sort now (NUM_PLAN_KINDS stays what it counted when kind 11 came)
constexpr uint32_t NUM_WIDE_KINDS = 14;  // with KIND_LONGDIV_WIDE: the key width of finish_plan's counting sort now (NUM_HINT_KINDS stays what it counted when kind 12 came)
constexpr uint32_t NUM_MULDIV_KINDS = 15;  // with KIND_MODMULDIV: the key width of finish_plan's counting sort now (NUM_WIDE_KINDS stays what it counted when kind 13 came)
constexpr uint32_t MAX_BLOCK = 64;       // the largest linear block: one wave, a lane per row and per column

// What a launch does with its steps [lo, hi): LAUNCH_CHAIN, one lane per assignment walks them in order, through consecutive narrow
// levels; every other kind, one lane (LAUNCH_BLOCK and LAUNCH_LONGDIV_WIDE: one wave) per (step, assignment), and every step has the
// step kinds that KIND_INFO maps to that launch kind, all of one level.  LAUNCH_LEVEL: the ordinary steps.
enum LaunchKind : uint8_t { LAUNCH_CHAIN, LAUNCH_LEVEL, LAUNCH_BITS, LAUNCH_ISZERO, LAUNCH_DIVREM, LAUNCH_INDICATOR, LAUNCH_SQRT,
                            LAUNCH_BLOCK, LAUNCH_LONGDIV, LAUNCH_MODDIV, LAUNCH_LONGDIV_WIDE, LAUNCH_MODMULDIV };

// What "a kind of step" means to the schedule, per step kind: the launch kind it gets in a wide level; whether it counts as dividing
// (KIND_DIVREM for 1 / cq, KIND_SQRT for 1 / (ka kb); KIND_INDICATOR, the blocks and the declared hints do not); whether one lane can
// walk it in a chain (the blocks and the wide hints take a wave, the hints a launch's trip counts: always launches of their own).
// finish_plan builds the launches from it, the driver and the CPU rig check a plan against it.
struct KindInfo {
    uint8_t launch, divides, chained;
};
constexpr KindInfo KIND_INFO[NUM_MULDIV_KINDS] = {
    {LAUNCH_LEVEL, 0, 1},      // KIND_C
    {LAUNCH_LEVEL, 1, 1},      // KIND_A
    {LAUNCH_LEVEL, 1, 1},      // KIND_B
    {LAUNCH_BITS, 0, 1},       // KIND_BITS_C
    {LAUNCH_BITS, 1, 1},       // KIND_BITS_A
    {LAUNCH_BITS, 1, 1},       // KIND_BITS_B
    {LAUNCH_ISZERO, 1, 1},     // KIND_ISZERO
    {LAUNCH_DIVREM, 1, 1},     // KIND_DIVREM
    {LAUNCH_INDICATOR, 0, 1},  // KIND_INDICATOR
    {LAUNCH_SQRT, 1, 1},       // KIND_SQRT
    {LAUNCH_BLOCK, 0, 0},      // KIND_BLOCK
    {LAUNCH_LONGDIV, 0, 0},    // KIND_LONGDIV
    {LAUNCH_MODDIV, 0, 0},     // KIND_MODDIV
    {LAUNCH_LONGDIV_WIDE, 0, 0},  // KIND_LONGDIV_WIDE
    {LAUNCH_MODMULDIV, 0, 0},  // KIND_MODMULDIV
};

constexpr uint8_t PATTERN_UNKNOWN = 1, PATTERN_QUOTIENT = 2, PATTERN_INDICATOR = 3, PATTERN_SQRT = 4;   // the pattern bytes (0: given)

constexpr uint32_t WIDE_STEPS = 32;   // a level of at least this many steps gets launches of its own; narrower ones are walked by one lane per assignment

struct Csr {
    const uint64_t *rowptr;   // nr + 1
    const uint32_t *col;      // nnz
    const uint64_t *val;      // nnz x 4 words; all four zero = a zero coefficient
};

struct Step {
    uint64_t pos;     // index of the unknown's entry in its matrix (col / val arrays); a decomposition: of the entry that holds c
    uint32_t row, col, kind, level;
    uint32_t bits = 0, cols_off = 0;   // a decomposition: Plan::bit_cols[cols_off .. cols_off + bits), exponent order; bits = 0 otherwise
                                       // an is-zero pair: row = the closer, pos / col = the flag's entry in it, Plan::pairs[cols_off]
                                       // a division row: pos / col = the quotient's entry in A_r or B_r, Plan::divs[cols_off]
                                       // an indicator row: pos / col = the indicator's entry, cols_off = 1: it lies in B_r and K = A_r; 0: the other way round
                                       // a square-root row: pos / col = the root's entry in A_r, cols_off = the offset of its entry in B_r from that row's start
                                       // a linear block: row / col = its smallest row and column, pos = 0, Plan::blocks[cols_off]
};

struct PairRows {     // what an is-zero step needs beside its Step
    uint64_t pos_m, pos_c;   // the multiplier's entry in A_r1 or B_r1; the flag's entry in C_r1
    uint32_t row1, col_m;    // the opener; the multiplier's column
    uint8_t m_in_b;          // 1: the multiplier lies in B_r1 and K1 = A_r1; 0: the other way round
    uint8_t b_in_b;          // 1: the flag lies in B_r2 and K2 = A_r2
    uint8_t negated;         // 1: K2 = -K1
};

struct DivRow {       // what a division step needs beside its Step
    uint64_t pos_r;          // the remainder's entry in C_r
    uint32_t col_r;          // the remainder's column
    uint8_t q_in_b;          // 1: the quotient lies in B_r and K = A_r; 0: the other way round
};

struct BlockRows {    // what a block step needs beside its Step
    std::vector<uint32_t> rows, cols;   // k rows and k columns, both ascending
    uint32_t mat;                       // Plan::block_mats[mat]
};

struct BlockMat {     // a distinct block matrix
    uint32_t k;
    std::vector<uint64_t> words;        // k x k coefficients of 4 words, row-major: M[i][j] = the coefficient of cols[j] in C_{rows[i]}
};

// A declared hint (pm_pk_set_hints): limb-wise long division.  Columns are CSR columns (0: the constant one, then the instance, then
// the witness).  `lit`: with HINT_DIVISOR_LITERAL the divisor's kE limbs as canonical integers of four words each, and E is empty.
constexpr uint64_t HINT_LONGDIV = 1, HINT_DIVISOR_LITERAL = 1;
// the modular division's opcode (2 stays reserved and refused), its flag and the limits of its record: kz outputs, kP modulus limbs,
// at most 32 limbs in each of N+, N-, D+, D-; every operand sum below 2^1024, the modulus below 2^512
constexpr uint64_t HINT_MODDIV = 3, HINT_MODULUS_LITERAL = 1;
constexpr uint32_t MODDIV_MAX_KZ = 16, MODDIV_MAX_KP = 16, MODDIV_MAX_K = 32, MODDIV_OPERAND_BITS = 1024, MODDIV_MODULUS_BITS = 512;
// the wide long division's opcode (4 is refused as unknown, like 2) and the limits of its record; its flag is HINT_DIVISOR_LITERAL
constexpr uint64_t HINT_LONGDIV_WIDE = 5;
constexpr uint32_t WIDE_MAX_KD = 128, WIDE_MAX_KE = 64, WIDE_MAX_KQ = 128, WIDE_MAX_KR = 64, WIDE_D_BITS = 8192, WIDE_E_BITS = 4096;
// the modular multiply-divide's opcode (6 is refused as unknown, like 2 and 4) and the limits of its record: kz, kP and the addend and
// denominator lists as opcode 3's, at least one and at most 32 limbs in each factor; its flag is HINT_MODULUS_LITERAL, its operand and
// modulus bounds MODDIV_OPERAND_BITS and MODDIV_MODULUS_BITS; cN and cD are literals of one 32-bit word, not zero
constexpr uint64_t HINT_MODMULDIV = 7, MODMULDIV_MAX_C = 0xffffffffull;
constexpr uint32_t MODMULDIV_LISTS = 6;
constexpr uint32_t HINT_MAX_N = 128, HINT_MAX_KD = 32, HINT_MAX_KE = 16, HINT_MAX_KQ = 32, HINT_MAX_KR = 16, HINT_D_BITS = 1024, HINT_E_BITS = 512;
struct Hint {
    uint32_t n = 0, flags = 0;
    std::vector<uint32_t> q, rem, D, E;
    std::vector<uint64_t> lit;
    uint32_t index = 0;                 // its place in the declaration: the stuck word is nr + index
    // A MODULAR DIVISION (op == HINT_MODDIV) uses the same lists, so that the scheduler reads both opcodes alike: q = the kz output
    // columns, rem empty, D = the kNp + kNm numerator columns followed by the kDp + kDm denominator columns, E = the kP modulus
    // columns (lit: its literal limbs, with HINT_MODULUS_LITERAL); k[4] = kNp, kNm, kDp, kDm, the parts of D
    // A WIDE long division (op == HINT_LONGDIV_WIDE) uses the lists exactly as a long division does
    uint32_t op = (uint32_t)HINT_LONGDIV;
    uint32_t k[4] = {0, 0, 0, 0};
    // A MODULAR MULTIPLY-DIVIDE (op == HINT_MODMULDIV) uses the lists in the same way: q = the kz output columns, rem empty, D = the six
    // operand lists one after the other -- kA, kB factor columns, kNp, kNm addend columns, kDp, kDm denominator columns --, E = the kP
    // modulus columns (lit: its literal limbs); km[6] = kA, kB, kNp, kNm, kDp, kDm, the parts of D (k[4] stays zero: opcode 3 alone
    // reads it); c[2] = cN, cD
    uint32_t km[MODMULDIV_LISTS] = {0, 0, 0, 0, 0, 0};
    uint32_t c[2] = {1, 1};
};

struct Launch {
    uint32_t lo, hi;  // steps [lo, hi) of the sorted list
    uint8_t kind;     // a LaunchKind
    uint8_t divides;  // 1: some step of the range has a kind that KIND_INFO counts as dividing
    uint32_t rounds = 0;    // the hint kinds only.  LAUNCH_LONGDIV: the division's trip count, the largest min(1024, n (kD - 1) + 256)
                            // of the range's hints -- a dividend of kD limbs below 2^256 at bit offsets n j is below 2 to that power;
                            // LAUNCH_MODDIV: the same bound over the four operand lists of the range's hints (the reductions modulo P);
                            // LAUNCH_LONGDIV_WIDE: the largest min(8192, n (kD - 1) + 256) of the range's hints: a bound that sizes the
                            // wave's arrays, not a trip count
                            // LAUNCH_MODMULDIV: LAUNCH_MODDIV's bound over the six operand lists of the range's hints
    uint32_t inv_rounds = 0;// LAUNCH_MODDIV and LAUNCH_MODMULDIV (where it is the trip count of the product's reduction as well):
                            // the inversion's trip count 2 L, L the largest min(512, n (kP - 1) + 256) of the range's hints:
                            // every modulus of the range that is not stuck is below 2^L (solve_steps.cuh: modinv_odd proves the bound)
};

enum Error : int { OK = 0, ERR_MANY_UNKNOWNS = 1, ERR_TWO_MATRICES = 2, ERR_UNDETERMINED = 3, ERR_COLUMN_ZERO = 4, ERR_HINT = 5 };

struct Plan {
    std::vector<Step> steps;          // sorted by (level, kind, row)
    std::vector<uint32_t> level_ptr;  // level l (1-based) = steps [level_ptr[l - 1], level_ptr[l])
    std::vector<Launch> launches;
    std::vector<uint32_t> bit_cols;   // the decompositions' columns
    std::vector<PairRows> pairs;      // the is-zero pairs' openers, in order of discovery
    std::vector<DivRow> divs;         // the division rows' remainders, in order of discovery
    std::vector<BlockRows> blocks;    // the linear blocks, in order of discovery
    std::vector<BlockMat> block_mats; // their distinct matrices, in order of discovery
    std::vector<Hint> hints;          // the declared hints that acted, in order of discovery
    int error = OK;
    uint64_t error_row = 0, error_col = 0;
    std::string message;              // empty when error == OK
    bool reordered = false;           // build_plan_any_order: the steps do not follow the matrix order (the stuck word needs the level then)
    uint32_t levels() const { return level_ptr.empty() ? 0 : (uint32_t)level_ptr.size() - 1; }
};

inline bool coef_is_zero(const uint64_t *v) { return (v[0] | v[1] | v[2] | v[3]) == 0; }

// 256-bit helpers on canonical residues (4 x u64, little-endian)
inline bool words_less(const uint64_t *a, const uint64_t *b) {
    for (int i = 3; i >= 0; --i)
        if (a[i] != b[i]) return a[i] < b[i];
    return false;
}
inline bool words_equal(const uint64_t *a, const uint64_t *b) { return a[0] == b[0] && a[1] == b[1] && a[2] == b[2] && a[3] == b[3]; }
// out = a + b mod `modulus`, for a, b < modulus
inline void add_mod(const uint64_t *a, const uint64_t *b, const uint64_t *modulus, uint64_t *out) {
    uint64_t s[4], d[4], carry = 0, borrow = 0;
    for (int i = 0; i < 4; ++i) {
        const uint64_t t = a[i] + carry;
        const uint64_t c1 = t < carry;
        s[i] = t + b[i];
        carry = c1 | (uint64_t)(s[i] < t);
    }
    for (int i = 0; i < 4; ++i) {
        const uint64_t t = s[i] - borrow;
        const uint64_t b1 = s[i] < borrow;
        d[i] = t - modulus[i];
        borrow = b1 | (uint64_t)(t < modulus[i]);
    }
    const bool ge = carry || !borrow;
    for (int i = 0; i < 4; ++i) out[i] = ge ? d[i] : s[i];
}
inline uint32_t bit_length(const uint64_t *a) {
    for (int i = 3; i >= 0; --i)
        if (a[i]) return 64 * (uint32_t)i + 64 - (uint32_t)__builtin_clzll(a[i]);
    return 0;
}

struct Unknown {   // an unknown's entry in the row under the cursor
    uint32_t matrix, col;
    uint64_t pos;
};

// the booleanity shape, for a row whose unknown entries are `occ` (all of one column) with nz[k] non-zero entries in matrix k
inline bool is_booleanity(const Csr m[3], uint64_t r, const std::vector<Unknown> &occ, const uint32_t nz[3], const uint64_t *modulus) {
    if (occ.size() != 2 || occ[0].matrix != 0 || occ[1].matrix != 1 || nz[2] != 0) return false;
    if (!((nz[0] == 1 && nz[1] == 2) || (nz[0] == 2 && nz[1] == 1))) return false;
    const int two = nz[0] == 2 ? 0 : 1;   // the side k' (1 - z_u)
    for (uint64_t e = m[two].rowptr[r]; e < m[two].rowptr[r + 1]; ++e) {
        if (e == occ[two].pos || coef_is_zero(m[two].val + 4 * e)) continue;
        uint64_t sum[4];
        add_mod(m[two].val + 4 * e, m[two].val + 4 * occ[two].pos, modulus, sum);
        return m[two].col[e] == 0 && coef_is_zero(sum);
    }
    return false;
}

// the decomposition shape, for a row whose unknown entries are `occ` (two or more columns): nullptr and `order` = the indices of
// occ in exponent order, or the condition that failed
inline const char *decomposition_order(const Csr m[3], const std::vector<Unknown> &occ, const std::vector<uint32_t> &bool_row, const uint64_t *modulus,
                                       std::vector<uint32_t> &order) {
    constexpr uint32_t NONE = ~(uint32_t)0;
    const size_t k = occ.size();
    for (const Unknown &o : occ) {
        if (o.matrix != occ[0].matrix) return "the unknowns lie in more than one matrix";
        if (bool_row[o.col] == NONE) return "an unknown that no earlier row constrains boolean";
    }
    if (k > bit_length(modulus) - 1) return "more bits than bitlength(r) - 1";
    const uint64_t *val = m[occ[0].matrix].val;
    std::vector<uint32_t> sorted(k), next(k, NONE);
    for (size_t i = 0; i < k; ++i) sorted[i] = (uint32_t)i;
    const auto less = [&](uint32_t a, uint32_t b) { return words_less(val + 4 * occ[a].pos, val + 4 * occ[b].pos); };
    std::sort(sorted.begin(), sorted.end(), less);
    for (size_t i = 1; i < k; ++i)
        if (words_equal(val + 4 * occ[sorted[i - 1]].pos, val + 4 * occ[sorted[i]].pos)) return "a coefficient occurs twice";
    std::vector<uint8_t> has_pred(k, 0);
    for (size_t i = 0; i < k; ++i) {
        uint64_t twice[4];
        add_mod(val + 4 * occ[i].pos, val + 4 * occ[i].pos, modulus, twice);
        const auto it = std::lower_bound(sorted.begin(), sorted.end(), twice, [&](uint32_t a, const uint64_t *w) { return words_less(val + 4 * occ[a].pos, w); });
        if (it != sorted.end() && words_equal(val + 4 * occ[*it].pos, twice)) {
            next[i] = *it;
            has_pred[*it] = 1;
        }
    }
    uint32_t first = NONE;
    for (size_t i = 0; i < k; ++i)
        if (!has_pred[i]) {
            if (first != NONE) return "the coefficients are not c 2^0 ... c 2^(k-1)";
            first = (uint32_t)i;
        }
    order.clear();
    for (uint32_t i = first; i != NONE && order.size() < k; i = next[i]) order.push_back(i);
    return order.size() == k ? nullptr : "the coefficients are not c 2^0 ... c 2^(k-1)";
}

struct Opener {   // an is-zero opener whose closer has not come yet
    uint64_t pos_m, pos_c;
    uint32_t row, col_m, col_b, reads;   // reads: the largest level among the columns the row reads
    uint8_t m_in_b;
};

// K2 (matrix k2, row r2) against K1 (matrix k1, row r1) as linear combinations: 0 equal, 1 every coefficient negated, -1 neither.
// Neither side names an unknown; zero coefficients name nothing.  `a`, `b`: scratch.
inline int compare_known_sides(const Csr m[3], int k1, uint64_t r1, int k2, uint64_t r2, const uint64_t *modulus, std::vector<std::pair<uint32_t, uint64_t>> &a,
                               std::vector<std::pair<uint32_t, uint64_t>> &b) {
    const auto gather = [&](int k, uint64_t r, std::vector<std::pair<uint32_t, uint64_t>> &out) {
        out.clear();
        for (uint64_t e = m[k].rowptr[r]; e < m[k].rowptr[r + 1]; ++e)
            if (!coef_is_zero(m[k].val + 4 * e)) out.push_back({m[k].col[e], e});
        std::sort(out.begin(), out.end());
    };
    gather(k1, r1, a);
    gather(k2, r2, b);
    if (a.size() != b.size()) return -1;
    bool same = true, negated = true;
    for (size_t i = 0; i < a.size(); ++i) {
        if (a[i].first != b[i].first) return -1;
        const uint64_t *va = m[k1].val + 4 * a[i].second, *vb = m[k2].val + 4 * b[i].second;
        uint64_t sum[4];
        add_mod(va, vb, modulus, sum);
        same = same && words_equal(va, vb);
        negated = negated && coef_is_zero(sum);
    }
    return same ? 0 : negated ? 1 : -1;
}

// The division shape, for a row whose unknown entries are `occ` (two or more columns) with nz[k] non-zero entries in matrix k:
//   0   no byte-2 column is the lone entry of A_r or B_r: the row is no candidate
//   1   a division row: `q` = the quotient's entry, `rem` = the remainder's entry in C_r
//  -1   a candidate that misses a condition: `why`
inline int division_row(const Csr m[3], const std::vector<Unknown> &occ, const uint32_t nz[3], const uint8_t *unknown, const uint64_t *modulus, Unknown &q,
                        Unknown &rem, const char *&why) {
    const Unknown *lone = nullptr;
    for (const Unknown &e : occ)
        if (!lone && e.matrix < 2 && nz[e.matrix] == 1 && unknown[e.col] == PATTERN_QUOTIENT) lone = &e;
    if (!lone) return 0;
    q = *lone;
    const uint32_t other_side = 1 - q.matrix;
    const Unknown *first = nullptr;
    uint32_t named = 0;
    bool in_ab = false, third = false;
    for (const Unknown &e : occ) {
        if (&e == lone) continue;
        if (e.col == q.col) return why = "the quotient named twice", -1;
        if (!first) first = &e;
        third = third || e.col != first->col;
        ++named;
        in_ab = in_ab || e.matrix < 2;      // the quotient's side has no other non-zero entry: this is the other side
    }
    if (third) return why = in_ab ? "the other side not known" : "a third unknown", -1;
    if (in_ab) return why = "rem in A or B", -1;
    if (named > 1) return why = "rem named twice", -1;
    if (nz[other_side] == 0) return why = "the other side not known", -1;
    rem = *first;
    uint64_t sum[4];
    add_mod(m[q.matrix].val + 4 * q.pos, m[2].val + 4 * rem.pos, modulus, sum);
    if (!coef_is_zero(sum)) return why = "cr != -cq", -1;
    return 1;
}

// The indicator shape, for a row whose ONLY unknown entry is `e` (named once) with nz[k] non-zero entries in matrix k: the column
// carries byte 3, it is the lone non-zero entry of A_r or B_r, the other of the two is the known guard side K (no unknown -- there
// is none left -- and at least one non-zero entry) and C_r has no non-zero entry.  Any other shape is an ordinary step.
inline bool indicator_row(const Unknown &e, const uint32_t nz[3], const uint8_t *unknown) {
    return unknown[e.col] == PATTERN_INDICATOR && e.matrix < 2 && nz[e.matrix] == 1 && nz[1 - e.matrix] >= 1 && nz[2] == 0;
}
inline Step indicator_step(const Unknown &e, uint32_t r, uint32_t lv) {
    Step s{e.pos, r, e.col, KIND_INDICATOR, lv};
    s.cols_off = e.matrix;   // 1: the indicator lies in B_r and K = A_r
    return s;
}

// The square-root shape, for a row whose unknown entries `occ` are all of ONE column with nz[k] non-zero entries in matrix k: the
// column carries byte 4 and is named exactly twice, as the lone non-zero entry of A_r and the lone non-zero entry of B_r (so C_r names
// no unknown: there is none left).  Any other shape is what it was without the marker.
inline bool sqrt_row(const std::vector<Unknown> &occ, const uint32_t nz[3], const uint8_t *unknown) {
    return occ.size() == 2 && occ[0].matrix == 0 && occ[1].matrix == 1 && unknown[occ[0].col] == PATTERN_SQRT && nz[0] == 1 && nz[1] == 1;
}

// The trip-count bounds of a hint launch over its steps (Launch::rounds, Launch::inv_rounds); a launch of any other kind keeps zero
inline void hint_rounds(const Plan &p, Launch &l) {
    if (l.kind != LAUNCH_LONGDIV && l.kind != LAUNCH_MODDIV && l.kind != LAUNCH_LONGDIV_WIDE && l.kind != LAUNCH_MODMULDIV) return;
    for (uint32_t t = l.lo; t < l.hi; ++t) {
        const Hint &h = p.hints[p.steps[t].cols_off];
        if (l.kind == LAUNCH_MODDIV || l.kind == LAUNCH_MODMULDIV) {
            for (uint32_t k : h.k)
                if (k) l.rounds = std::max(l.rounds, std::min(h.n * (k - 1) + 256, MODDIV_OPERAND_BITS));
            for (uint32_t k : h.km)
                if (k) l.rounds = std::max(l.rounds, std::min(h.n * (k - 1) + 256, MODDIV_OPERAND_BITS));
            const uint32_t kP = (uint32_t)(h.flags & HINT_MODULUS_LITERAL ? h.lit.size() / 4 : h.E.size());
            l.inv_rounds = std::max(l.inv_rounds, 2 * std::min(h.n * (kP - 1) + 256, MODDIV_MODULUS_BITS));
        } else {
            l.rounds = std::max(l.rounds, std::min(h.n * ((uint32_t)h.D.size() - 1) + 256, l.kind == LAUNCH_LONGDIV ? HINT_D_BITS : WIDE_D_BITS));
        }
    }
}

// The tail both builders share: p.steps (in ROW order, levels set) sorted by (level, kind), stable by row; level_ptr; the launch schedule.
inline void finish_plan(Plan &p, uint32_t max_level, uint32_t wide_steps) {
    // counting sort by (level, kind); the row order inside a key is the order the steps come in
    constexpr size_t K = NUM_MULDIV_KINDS;
    std::vector<uint32_t> start((size_t)max_level * K + 1, 0);
    for (const Step &s : p.steps) ++start[(size_t)(s.level - 1) * K + s.kind + 1];
    for (size_t i = 1; i < start.size(); ++i) start[i] += start[i - 1];
    p.level_ptr.resize((size_t)max_level + 1);
    for (uint32_t l = 0; l <= max_level; ++l) p.level_ptr[l] = start[(size_t)l * K];
    {
        std::vector<Step> sorted(p.steps.size());
        std::vector<uint32_t> cursor(start.begin(), start.end() - 1);
        for (const Step &s : p.steps) sorted[cursor[(size_t)(s.level - 1) * K + s.kind]++] = s;
        p.steps.swap(sorted);
    }
    // launch schedule, read from KIND_INFO.  The kinds that one lane can walk come first in a level.  Where they are a wide run, each
    // gets the launch of its kind, adjacent kinds with the same launch kind and the same `divides` sharing one (so a level splits where
    // the dividing kinds begin, again where the decompositions and their dividing kinds begin, then per kind; the indicator rows do not
    // divide, the square-root rows do); where they are narrow, consecutive levels are one chain, which divides if any kind in it does (a
    // chain of C-steps and indicators is a non-dividing one).  The other kinds come last and are launches of their own whatever the
    // level's width (a wave per block, not a lane): a chain run ends before them and a new one begins after them.  First the linear
    // blocks, then the declared hints: the long divisions, the modular divisions, the wide long divisions, the modular multiply-divides
    for (uint32_t l = 0; l < max_level; ++l) {
        const uint32_t *at = start.data() + (size_t)l * K;
        uint32_t walked = 0;   // the kinds of the chainable run
        uint8_t divides = 0;
        for (; walked < K && KIND_INFO[walked].chained; ++walked)
            if (at[walked + 1] > at[walked]) divides |= KIND_INFO[walked].divides;
        const uint32_t lo = at[0], hi = at[walked];
        const bool wide = hi - lo >= wide_steps;
        if (hi == lo || wide) {
            // nothing for a chain: a level of blocks and hints only, or a wide one
        } else if (!p.launches.empty() && p.launches.back().kind == LAUNCH_CHAIN) {
            p.launches.back().hi = hi;
            p.launches.back().divides |= divides;
        } else {
            p.launches.push_back(Launch{lo, hi, LAUNCH_CHAIN, divides});
        }
        for (uint32_t a = wide ? 0 : walked, b; a < K; a = b) {
            const KindInfo &info = KIND_INFO[a];
            for (b = a + 1; b < K && KIND_INFO[b].launch == info.launch && KIND_INFO[b].divides == info.divides;) ++b;
            if (at[b] == at[a]) continue;
            Launch own{at[a], at[b], info.launch, info.divides};
            hint_rounds(p, own);
            p.launches.push_back(own);
        }
    }
}

constexpr uint32_t KIND_OF[3] = {KIND_A, KIND_B, KIND_C};   // the ordinary kind of an unknown in matrix A, B, C

// What both builders keep while they walk the rows -- the column state, the openers, the plan under construction, the row under the
// cursor -- and every rule they share, each stated once: how a row is read, which shape opens a pair, and how each kind of step is
// made.  A step's constructor sets the levels of the columns it determines and max_level, and calls `known` (its last argument) with
// each of those columns: in matrix order nobody listens, in the scheduler the rows parked on the column return to the heap.
struct Planner {
    static constexpr uint32_t UNSOLVED = ~(uint32_t)0, NONE = ~(uint32_t)0;
    const Csr *m;
    const uint8_t *unknown;
    const uint64_t *modulus;
    Plan p;
    std::vector<uint32_t> level;      // per column: 0 given, UNSOLVED, or the level of the step that determines it
    std::vector<uint32_t> bool_row;   // boolean-pending: the column is UNSOLVED and this is its booleanity row
    std::vector<uint32_t> pair_of;    // pair-pending: the column is UNSOLVED and this is its entry of `openers`
    std::vector<Opener> openers;
    size_t open = 0;                  // openers not closed yet
    uint32_t max_level = 0;
    // the row under the cursor (read_row)
    std::vector<Unknown> occ;         // its unknown entries, A then B then C, in stored order
    uint32_t reads = 0, nz[3] = {0, 0, 0};   // the largest level among the columns it reads; its non-zero entries per matrix
    std::vector<uint32_t> order;      // scratch: decomposition_order
    std::vector<std::pair<uint32_t, uint64_t>> side1, side2;   // scratch: compare_known_sides

    Planner(const Csr *matrices, uint64_t ncols, const uint8_t *pattern, const uint64_t *mod)
        : m(matrices), unknown(pattern), modulus(mod), level(ncols), bool_row(mod ? ncols : 0, NONE), pair_of(mod ? ncols : 0, NONE) {
        for (uint64_t j = 0; j < ncols; ++j) level[j] = unknown[j] ? UNSOLVED : 0;
    }

    // occ, nz and reads of row r.  whole = false stops at the second unknown entry (nz and reads are then incomplete)
    void read_row(uint64_t r, bool whole) {
        reads = 0;
        nz[0] = nz[1] = nz[2] = 0;
        occ.clear();
        for (int k = 0; k < 3 && (whole || occ.size() < 2); ++k) {
            for (uint64_t e = m[k].rowptr[r]; e < m[k].rowptr[r + 1] && (whole || occ.size() < 2); ++e) {
                if (coef_is_zero(m[k].val + 4 * e)) continue;
                ++nz[k];
                const uint32_t j = m[k].col[e];
                if (level[j] != UNSOLVED) {
                    if (level[j] > reads) reads = level[j];
                    continue;
                }
                occ.push_back(Unknown{(uint32_t)k, j, e});
            }
        }
    }
    // the pending opener that the row's first pair-pending unknown belongs to
    const Opener *pending_opener() const {
        for (const Unknown &e : occ)
            if (pair_of[e.col] != NONE) return &openers[pair_of[e.col]];
        return nullptr;
    }
    // an is-zero opener: two unknowns, the multiplier alone on one of A, B, the other of the two known and not zero, the flag in C
    bool opener_shape() const {
        return occ.size() == 2 && occ[0].col != occ[1].col && occ[0].matrix < 2 && occ[1].matrix == 2 && nz[occ[0].matrix] == 1 && nz[1 - occ[0].matrix] >= 1;
    }
    void register_opener(uint32_t r) {
        pair_of[occ[0].col] = pair_of[occ[1].col] = (uint32_t)openers.size();
        openers.push_back(Opener{occ[0].pos, occ[1].pos, r, occ[0].col, occ[1].col, reads, (uint8_t)occ[0].matrix});
        ++open;
    }
    // the opener is none after all, or its pair is closed: its columns are pair-pending no longer
    void drop_opener(const Opener &o) {
        pair_of[o.col_m] = pair_of[o.col_b] = NONE;
        --open;
    }
    void solved(uint32_t col, uint32_t lv) {
        level[col] = lv;
        if (lv > max_level) max_level = lv;
    }

    // the row's single unknown e, named once: an ordinary step, or -- byte 3 on it and the indicator shape -- the indicator step
    template <class Known>
    void single_step(const Unknown &e, uint32_t r, const Known &known) {
        const uint32_t lv = reads + 1;
        p.steps.push_back(modulus && indicator_row(e, nz, unknown) ? indicator_step(e, r, lv) : Step{e.pos, r, e.col, KIND_OF[e.matrix], lv});
        solved(e.col, lv);
        known(e.col);
    }
    // a square-root row (sqrt_row): occ = u's entry in A_r, then its entry in B_r
    template <class Known>
    void sqrt_step(uint32_t r, const Known &known) {
        const uint32_t lv = reads + 1, col = occ[0].col;
        Step s{occ[0].pos, r, col, KIND_SQRT, lv};
        s.cols_off = (uint32_t)(occ[1].pos - m[1].rowptr[r]);
        p.steps.push_back(s);
        solved(col, lv);
        known(col);
    }
    // a decomposition whose exponent order is `order` (decomposition_order)
    template <class Known>
    void bits_step(uint32_t r, const Known &known) {
        const uint32_t lv = reads + 1;
        const Unknown &c = occ[order[0]];
        Step s{c.pos, r, c.col, KIND_BITS_C + KIND_OF[c.matrix], lv};
        s.bits = (uint32_t)order.size();
        s.cols_off = (uint32_t)p.bit_cols.size();
        for (uint32_t i : order) {
            p.bit_cols.push_back(occ[i].col);
            solved(occ[i].col, lv);
        }
        p.steps.push_back(s);
        for (uint32_t i : order) known(occ[i].col);
    }
    // a division row with quotient q and remainder rem (division_row)
    template <class Known>
    void division_step(const Unknown &q, const Unknown &rem, uint32_t r, const Known &known) {
        const uint32_t lv = reads + 1;
        Step s{q.pos, r, q.col, KIND_DIVREM, lv};
        s.cols_off = (uint32_t)p.divs.size();
        p.divs.push_back(DivRow{rem.pos, rem.col, (uint8_t)(q.matrix == 1)});
        p.steps.push_back(s);
        solved(q.col, lv);
        solved(rem.col, lv);
        known(q.col);
        known(rem.col);
    }
    // row r closes the pair of opener o: `flag` is the flag's entry in it, sign = compare_known_sides (0: K2 = K1, 1: K2 = -K1)
    template <class Known>
    void iszero_step(const Opener &o, const Unknown &flag, uint32_t r, int sign, const Known &known) {
        const uint32_t lv = (reads > o.reads ? reads : o.reads) + 1, col_m = o.col_m, col_b = o.col_b;
        Step s{flag.pos, r, col_b, KIND_ISZERO, lv};
        s.cols_off = (uint32_t)p.pairs.size();
        p.pairs.push_back(PairRows{o.pos_m, o.pos_c, o.row, col_m, o.m_in_b, (uint8_t)(flag.matrix == 1), (uint8_t)sign});
        p.steps.push_back(s);
        drop_opener(o);
        solved(col_m, lv);
        solved(col_b, lv);
        known(col_m);
        known(col_b);
    }
    // a linear row (the scheduler only): two or more unknown entries, every one in C_r, no column boolean-pending (pair-pending
    // columns have made the row wait before it comes here; the first-entry rule gives one entry per column)
    bool linear_row() const {
        if (occ.size() < 2) return false;
        for (const Unknown &e : occ)
            if (e.matrix != 2 || bool_row[e.col] != NONE) return false;
        return true;
    }
    // a linear block: `rows` (ascending) over the columns `cols` (ascending, all still unknown), `reads` the largest level the rows read
    template <class Known>
    void block_step(const std::vector<uint32_t> &rows, const std::vector<uint32_t> &cols, uint32_t reads_all, const Known &known) {
        const uint32_t lv = reads_all + 1, k = (uint32_t)cols.size();
        std::vector<uint64_t> words((size_t)k * k * 4, 0);
        for (uint32_t i = 0; i < k; ++i)
            for (uint64_t e = m[2].rowptr[rows[i]]; e < m[2].rowptr[rows[i] + 1]; ++e) {
                if (coef_is_zero(m[2].val + 4 * e) || level[m[2].col[e]] != UNSOLVED) continue;
                const size_t j = (size_t)(std::lower_bound(cols.begin(), cols.end(), m[2].col[e]) - cols.begin());
                std::copy(m[2].val + 4 * e, m[2].val + 4 * e + 4, words.begin() + ((size_t)i * k + j) * 4);
            }
        const auto found = mat_of.find(words);
        uint32_t mat;
        if (found != mat_of.end()) {
            mat = found->second;
        } else {
            mat = (uint32_t)p.block_mats.size();
            mat_of.emplace(words, mat);
            p.block_mats.push_back(BlockMat{k, std::move(words)});
        }
        Step s{0, rows[0], cols[0], KIND_BLOCK, lv};
        s.cols_off = (uint32_t)p.blocks.size();
        p.blocks.push_back(BlockRows{rows, cols, mat});
        p.steps.push_back(s);
        for (uint32_t col : cols) solved(col, lv);
        for (uint32_t col : cols) known(col);
    }
    // a declared hint whose inputs are all known: one step at 1 + max level of its inputs (`nr`: the system's rows)
    template <class Known>
    void hint_step(const Hint &h, uint64_t nr, const Known &known) {
        uint32_t lv = 0;
        for (const std::vector<uint32_t> *in : {&h.D, &h.E})
            for (uint32_t col : *in) lv = level[col] > lv ? level[col] : lv;
        ++lv;
        Step s{0, (uint32_t)(nr + h.index), h.q[0], h.op == HINT_MODDIV ? KIND_MODDIV : h.op == HINT_LONGDIV_WIDE ? KIND_LONGDIV_WIDE : h.op == HINT_MODMULDIV ? KIND_MODMULDIV : KIND_LONGDIV, lv};
        s.cols_off = (uint32_t)p.hints.size();
        p.hints.push_back(h);
        p.steps.push_back(s);
        for (const std::vector<uint32_t> *out : {&h.q, &h.rem})
            for (uint32_t col : *out) solved(col, lv);
        for (const std::vector<uint32_t> *out : {&h.q, &h.rem})
            for (uint32_t col : *out) known(col);
    }
    std::vector<uint8_t> owned;       // per column, with an active hint only: 1 = hint-owned (an output of an active hint)
    std::map<std::vector<uint64_t>, uint32_t> mat_of;   // a block matrix' words (k follows from their number) -> its index in Plan::block_mats
    // a row is refused where it stands: the steps of the rows before it stay in the plan, as they always did
    void refuse_row(int code, uint64_t row, uint64_t col, const std::string &message) {
        p.error = code;
        p.error_row = row;
        p.error_col = col;
        p.message = message;
    }
    // the system is refused: no part of a plan is left behind
    void fail(int code, uint64_t row, uint64_t col, const std::string &message) {
        refuse_row(code, row, col, message);
        p.steps.clear();
        p.bit_cols.clear();
        p.pairs.clear();
        p.divs.clear();
        p.blocks.clear();
        p.block_mats.clear();
        p.hints.clear();
    }
};

inline Plan build_plan(const Csr m[3], uint64_t nr, uint64_t m0, uint64_t mw, const uint8_t *unknown, uint32_t wide_steps = WIDE_STEPS,
                       const uint64_t *modulus = nullptr) {
    const uint64_t ncols = m0 + mw;
    constexpr uint32_t UNSOLVED = Planner::UNSOLVED, NONE = Planner::NONE;
    if (ncols && unknown[0]) {
        Plan p;
        p.error = ERR_COLUMN_ZERO;
        p.message = "column 0 (the constant one) is marked unknown";
        return p;
    }
    Planner st(m, ncols, unknown, modulus);
    const std::vector<Unknown> &occ = st.occ;
    const auto nobody = [](uint32_t) {};   // a column became known: in matrix order nobody waits for one
    static const char *const NAME[3] = {"A", "B", "C"};
    const auto two_unknowns = [](uint64_t r, uint32_t u, uint32_t j) {
        return "row " + std::to_string(r) + ": two or more unknowns (columns " + std::to_string(u) + " and " + std::to_string(j) + ")";
    };
    const auto refuse_pair = [&](const Opener &o, const std::string &why) {
        st.fail(ERR_MANY_UNKNOWNS, o.row, o.col_b, two_unknowns(o.row, o.col_m, o.col_b) + ", and no is-zero pair: " + why);
    };
    for (uint64_t r = 0; r < nr; ++r) {
        // without the modulus the second unknown entry decides the error, as it always did; with it the whole row is read
        st.read_row(r, modulus != nullptr);
        if (occ.empty()) continue;
        if (st.open) {   // the first row that names a pair-pending column closes that pair, or the pair is refused
            if (const Opener *o = st.pending_opener()) {
                const std::string here = "row " + std::to_string(r);
                const Unknown *flag = nullptr, *multiplier = nullptr, *other = nullptr;
                bool in_c = false, twice = false, same_matrix = false;
                for (const Unknown &e : occ) {
                    if (e.col == o->col_m) multiplier = &e;
                    else if (e.col != o->col_b) other = other ? other : &e;
                    else if (e.matrix == 2) in_c = true;
                    else if (flag) { twice = true; same_matrix = flag->matrix == e.matrix; }
                    else flag = &e;
                }
                const std::string flag_name = " names the flag (column " + std::to_string(o->col_b) + ")";
                std::string why;
                if (multiplier) why = here + " names the multiplier (column " + std::to_string(o->col_m) + ")";
                else if (other) why = here + " has a second unknown (column " + std::to_string(other->col) + ")";
                else if (in_c) why = here + flag_name + " in C";
                else if (twice) why = here + flag_name + (same_matrix ? std::string(" twice in ") + NAME[flag->matrix] : std::string(" in A and in B"));
                int sign = 0;
                if (why.empty()) {
                    sign = compare_known_sides(m, o->m_in_b ? 0 : 1, o->row, flag->matrix == 0 ? 1 : 0, r, modulus, st.side1, st.side2);
                    if (sign < 0) why = here + ": its known side is neither the opener's nor minus the opener's";
                }
                if (!why.empty()) {
                    refuse_pair(*o, why);
                    return std::move(st.p);
                }
                st.iszero_step(*o, *flag, (uint32_t)r, sign, nobody);
                continue;
            }
        }
        if (occ.size() == 1) {
            st.single_step(occ[0], (uint32_t)r, nobody);
            continue;
        }
        const uint32_t u = occ[0].col;
        uint32_t j = occ[1].col;
        const char *why = nullptr, *div_why = nullptr;
        if (modulus) {
            bool one_column = true;
            for (const Unknown &o : occ)
                if (one_column && o.col != u) {   // two or more unknowns: the error names the first other one, wherever u occurs again
                    one_column = false;
                    j = o.col;
                }
            if (one_column) {
                if (is_booleanity(m, r, occ, st.nz, modulus)) {
                    if (st.bool_row[u] == NONE) st.bool_row[u] = (uint32_t)r;
                    continue;
                }
                if (sqrt_row(occ, st.nz, unknown)) {   // u u = c with the fourth marker on u: the square-root step
                    st.sqrt_step((uint32_t)r, nobody);
                    continue;
                }
            } else if (!(why = decomposition_order(m, occ, st.bool_row, modulus, st.order))) {
                st.bits_step((uint32_t)r, nobody);
                continue;
            }
            // a division row: the shape below with the quotient's marker on the lone entry.  It is a step at once, or refused at once
            int div = 0;
            if (!one_column) {
                Unknown q, rem;
                div = division_row(m, occ, st.nz, unknown, modulus, q, rem, div_why);
                if (div > 0) {
                    st.division_step(q, rem, (uint32_t)r, nobody);
                    continue;
                }
                if (div < 0 && div_why[0] == 'c') why = nullptr;   // cr != -cq: the opener's shape, whose message had no second part
            }
            if (div == 0 && st.opener_shape()) {
                st.register_opener((uint32_t)r);
                continue;
            }
        }
        if (j != u) {
            std::string message = two_unknowns(r, u, j);
            if (why) message += std::string(", and no bit decomposition: ") + why;
            if (div_why) message += std::string(", and no division row: ") + div_why;
            st.refuse_row(ERR_MANY_UNKNOWNS, r, j, message);
        } else {   // the same unknown again: in another matrix, or a second time in this one
            st.refuse_row(ERR_TWO_MATRICES, r, j,
                          "row " + std::to_string(r) + ": unknown column " + std::to_string(j) + " occurs in " + NAME[occ[0].matrix] + " and in " + NAME[occ[1].matrix]);
        }
        return std::move(st.p);
    }
    if (st.open) {   // openers are pushed in row order: the first one still pending has the smallest row
        for (size_t i = 0; i < st.openers.size(); ++i)
            if (st.pair_of[st.openers[i].col_m] == i) {
                refuse_pair(st.openers[i], "no later row closes it");
                return std::move(st.p);
            }
    }
    if (modulus) {
        uint64_t pending = ncols;
        for (uint64_t j = 0; j < ncols; ++j)
            if (st.level[j] == UNSOLVED && st.bool_row[j] != NONE && (pending == ncols || st.bool_row[j] < st.bool_row[pending])) pending = j;
        if (pending != ncols) {
            const uint64_t row = st.bool_row[pending];
            st.fail(ERR_TWO_MATRICES, row, pending,
                    "row " + std::to_string(row) + ": unknown column " + std::to_string(pending) +
                        " occurs in A and in B (a booleanity row, and no later row determines the column)");
            return std::move(st.p);
        }
    }
    for (uint64_t j = 0; j < ncols; ++j)
        if (st.level[j] == UNSOLVED) {
            st.fail(ERR_UNDETERMINED, 0, j, "column " + std::to_string(j) + " is marked unknown and no row determines it");
            return std::move(st.p);
        }
    finish_plan(st.p, st.max_level, wide_steps);
    return std::move(st.p);
}

// The waiting-row scheduler of build_plan_any_order: the rules of build_plan (Planner) on the rows in DEPENDENCY order.  A min-heap of
// rows to examine (at first every row); a row that cannot act yet is parked on its unknown columns and returns to the heap when one of
// them becomes known, becomes boolean-pending or is released by its opener.  -> false and `why` where no order solves the system.
// st.p.steps come out in order of discovery, with their levels; st.max_level is set.
// `active`: the declared hints that are active in this call (build_plan_any_order), or nullptr.  Their outputs are hint-owned
// (Planner::owned), each waits on its unknown input columns and acts from the `ready` queue, before the next row is examined.
inline bool schedule_any_order(Planner &st, uint64_t nr, uint64_t ncols, std::string &why, const std::vector<Hint> *active = nullptr) {
    constexpr uint32_t UNSOLVED = Planner::UNSOLVED, NONE = Planner::NONE;
    enum : uint8_t { PARKED = 0, QUEUED = 1, DONE = 2 };
    const Csr *m = st.m;
    const uint64_t *modulus = st.modulus;
    const std::vector<Unknown> &occ = st.occ;
    std::vector<uint32_t> park_head(ncols, NONE);
    std::vector<std::pair<uint32_t, uint32_t>> parked;   // (row, next node of the same column)
    std::vector<uint8_t> state(nr, QUEUED);
    // the linear rows: a sorted set S of unknown columns -> its entry of set_rows, the (row, largest level it reads) registered under
    // exactly S; registered[r] = the set row r is registered under now (a row examined again with the same set is not counted twice)
    std::map<std::vector<uint32_t>, uint32_t> set_of;
    std::vector<std::vector<std::pair<uint32_t, uint32_t>>> set_rows;
    std::vector<uint32_t> registered, set;
    std::vector<uint32_t> rows(nr);
    for (uint64_t r = 0; r < nr; ++r) rows[r] = (uint32_t)r;   // ascending: a min-heap as it stands
    std::priority_queue<uint32_t, std::vector<uint32_t>, std::greater<uint32_t>> heap(std::greater<uint32_t>(), std::move(rows));
    const auto push = [&](uint32_t r) {
        if (state[r] != PARKED) return;
        state[r] = QUEUED;
        heap.push(r);
    };
    // the hints: how many unknown input columns each still waits on, and per column the hints that wait on it
    const size_t n_hints = active ? active->size() : 0;
    std::vector<uint32_t> hint_waits(n_hints, 0), ready;
    std::map<uint32_t, std::vector<uint32_t>> hint_waiters;
    for (size_t h = 0; h < n_hints; ++h) {
        std::vector<uint32_t> inputs((*active)[h].D);
        inputs.insert(inputs.end(), (*active)[h].E.begin(), (*active)[h].E.end());
        std::sort(inputs.begin(), inputs.end());
        inputs.erase(std::unique(inputs.begin(), inputs.end()), inputs.end());
        for (uint32_t col : inputs)
            if (st.level[col] == UNSOLVED) {
                ++hint_waits[h];
                hint_waiters[col].push_back((uint32_t)h);
            }
        if (!hint_waits[h]) ready.push_back((uint32_t)h);
    }
    const auto wake = [&](uint32_t col) {
        for (uint32_t i = park_head[col]; i != NONE; i = parked[i].second) push(parked[i].first);
        park_head[col] = NONE;
        if (n_hints && st.level[col] != UNSOLVED) {   // known, not merely boolean-pending or released: the hints that read it
            const auto at = hint_waiters.find(col);
            if (at == hint_waiters.end()) return;
            for (uint32_t h : at->second)
                if (--hint_waits[h] == 0) ready.push_back(h);
            hint_waiters.erase(at);
        }
    };
    const auto park = [&](uint32_t r) {
        state[r] = PARKED;
        for (const Unknown &e : occ) {
            parked.push_back({r, park_head[e.col]});
            park_head[e.col] = (uint32_t)parked.size() - 1;
        }
    };
    // the opener was none: its columns are free again, and it is examined again with the rows that wait on them.  Both columns are
    // woken here, also the one that the releasing row goes on to solve (its step wakes that column again and finds nobody parked):
    // every push happens before the next pop of the heap, so which of the two wakes a row makes no difference
    const auto release = [&](const Opener &held) {
        const uint32_t col_m = held.col_m, col_b = held.col_b, opener_row = held.row;
        st.drop_opener(held);
        state[opener_row] = PARKED;
        push(opener_row);
        wake(col_m);
        wake(col_b);
    };
    while (!heap.empty() || !ready.empty()) {
        if (!ready.empty()) {        // a hint whose inputs are all known acts: its outputs wake their waiters
            const uint32_t h = ready.back();
            ready.pop_back();
            st.hint_step((*active)[h], nr, wake);
            continue;
        }
        const uint32_t r = heap.top();
        heap.pop();
        st.read_row(r, true);
        state[r] = DONE;
        if (occ.empty()) continue;   // a check row
        if (n_hints) {               // no row solves a hint-owned column: the row waits for the hint
            bool waits = false;
            for (const Unknown &e : occ) waits = waits || st.owned[e.col];
            if (waits) {
                park(r);
                continue;
            }
        }
        const uint32_t u = occ[0].col;
        bool one_column = true;
        for (const Unknown &e : occ) one_column = one_column && e.col == u;
        Unknown q, rem;
        const char *div_why = nullptr;
        const int div = one_column ? 0 : division_row(m, occ, st.nz, st.unknown, modulus, q, rem, div_why);
        if (div > 0) {
            // a division row whose only unknowns are q and rem: a step at once.  It waits for no closer, so an opener registered over
            // one of its columns (the row rem * 1 = y has that shape) was none: it is released and examined again.  A candidate that
            // misses a condition waits like any other row (below)
            for (const uint32_t col : {q.col, rem.col})
                if (st.pair_of[col] != NONE) release(st.openers[st.pair_of[col]]);
            st.division_step(q, rem, r, wake);
            continue;
        }
        if (one_column && sqrt_row(occ, st.nz, st.unknown)) {
            // a square-root row whose only unknown is its root: a step at once.  An opener registered over the root (the row
            // x = u * s has that shape) was none: it is released and examined again, as for a division row
            if (st.pair_of[u] != NONE) release(st.openers[st.pair_of[u]]);
            st.sqrt_step(r, wake);
            continue;
        }
        const Opener *o = st.pending_opener();
        if (o && one_column && u == o->col_b) {   // the flag alone: the closer, or no order helps
            const int sign = occ.size() == 1 && occ[0].matrix < 2 ? compare_known_sides(m, o->m_in_b ? 0 : 1, o->row, occ[0].matrix == 0 ? 1 : 0, r, modulus, st.side1, st.side2) : -1;
            if (sign < 0) {
                why = "row " + std::to_string(r) + " names only the flag (column " + std::to_string(u) + ") of the pair that row " + std::to_string(o->row) + " opens and does not close it";
                return false;
            }
            st.iszero_step(*o, occ[0], r, sign, wake);
            continue;
        }
        if (o && one_column && occ.size() == 1 && u == o->col_m) {
            // the multiplier alone and once: this row determines it as an ordinary step, so the opener was no opener.  It is released
            // and examined again (its other unknown is then an ordinary kind-C step of it)
            release(*o);
            o = nullptr;
        }
        if (o) {   // the multiplier beside something else, a second unknown, another opener over a pending column: after the closer
            park(r);
            continue;
        }
        if (one_column) {
            if (occ.size() == 1) {
                st.single_step(occ[0], r, wake);
            } else if (is_booleanity(m, r, occ, st.nz, modulus)) {
                if (st.bool_row[u] == NONE) {
                    st.bool_row[u] = r;
                    wake(u);
                }
            } else {
                park(r);   // a later row may determine u: this one is a check row then
            }
            continue;
        }
        if (!decomposition_order(m, occ, st.bool_row, modulus, st.order)) {
            st.bits_step(r, wake);
            continue;
        }
        if (div == 0 && st.opener_shape()) {
            st.register_opener(r);
            continue;
        }
        if (st.linear_row()) {
            // a linear row over S: registered under the sorted S, once.  The |S|-th such row makes the block; a wider set only waits
            set.clear();
            for (const Unknown &e : occ) set.push_back(e.col);
            std::sort(set.begin(), set.end());
            if (std::adjacent_find(set.begin(), set.end()) == set.end()) {
                const auto at = set_of.emplace(set, (uint32_t)set_rows.size());
                if (at.second) set_rows.emplace_back();
                const uint32_t id = at.first->second;
                if (registered.empty()) registered.assign(nr, NONE);
                if (registered[r] != id) {
                    registered[r] = id;
                    set_rows[id].push_back({r, st.reads});
                }
                if (set.size() <= MAX_BLOCK && set_rows[id].size() == set.size()) {
                    std::vector<uint32_t> block_rows;
                    uint32_t reads = 0;
                    for (const auto &row : set_rows[id]) {
                        block_rows.push_back(row.first);
                        if (row.second > reads) reads = row.second;
                    }
                    std::sort(block_rows.begin(), block_rows.end());
                    st.block_step(block_rows, set, reads, wake);   // the other k - 1 rows wake and are check rows
                    continue;
                }
            }
        }
        park(r);
    }
    std::string unready;             // the first hint that never became ready, and its first input column (dividend, then divisor) that stays unknown
    for (size_t h = 0; h < n_hints && unready.empty(); ++h)
        for (const std::vector<uint32_t> *in : {&(*active)[h].D, &(*active)[h].E})
            for (uint32_t col : *in)
                if (unready.empty() && hint_waits[h] && st.level[col] == UNSOLVED)
                    unready = "hint " + std::to_string((*active)[h].index) + ": input column " + std::to_string(col) + " is never determined; ";
    for (uint64_t j = 0; j < ncols; ++j)
        if (st.level[j] == UNSOLVED) {
            why = unready + "column " + std::to_string(j) + " stays unknown";
            if (st.pair_of[j] != NONE) why += " (the pair that row " + std::to_string(st.openers[st.pair_of[j]].row) + " opens is never closed)";
            else if (st.bool_row[j] != NONE) why += " (boolean by row " + std::to_string(st.bool_row[j]) + ", and nothing determines it)";
            for (const auto &wide : set_of) {   // a set of linear rows too wide for a block, whose rows are linear rows over it to the end
                bool waits = wide.first.size() > MAX_BLOCK && std::binary_search(wide.first.begin(), wide.first.end(), (uint32_t)j);
                for (size_t i = 0; waits && i < wide.first.size(); ++i) {
                    const uint32_t col = wide.first[i];
                    waits = st.level[col] == UNSOLVED && st.bool_row[col] == NONE && st.pair_of[col] == NONE;
                }
                if (!waits) continue;
                why += ", and no linear block: " + std::to_string(wide.first.size()) + " unknowns exceed " + std::to_string(MAX_BLOCK);
                break;
            }
            return false;
        }
    return st.open == 0;
}

// The declaration of pm_pk_set_hints: `desc` is a sequence of records
//   HINT_LONGDIV, n, kq, kr, kD, kE, flags, kq quotient columns, kr remainder columns, kD dividend columns, then kE divisor columns
//   -- or, with HINT_DIVISOR_LITERAL (flags bit 0), kE limb values of four words each (canonical integers below r)
//   HINT_MODDIV, n, kz, kNp, kNm, kDp, kDm, kP, flags, kz output columns, kNp + kNm numerator columns, kDp + kDm denominator columns,
//   then kP modulus columns -- or, with HINT_MODULUS_LITERAL (flags bit 0), kP limb values of four words each
//   HINT_LONGDIV_WIDE, n, kq, kr, kD, kE, flags, and what follows HINT_LONGDIV's head: the same record under the wide limits
//   HINT_MODMULDIV, n, kz, kA, kB, kNp, kNm, kDp, kDm, kP, flags, cN, cD, kz output columns, kA + kB factor columns, kNp + kNm addend
//   columns, kDp + kDm denominator columns, then kP modulus columns -- or, with HINT_MODULUS_LITERAL, kP limb values of four words each
// in any mixture; both opcodes share the index h and the set of output columns.  Opcode 2 is reserved and refused like any unknown one.
// So does the third opcode; 4 is refused as unknown as well.  So does the fourth; 6 and 8 are refused as unknown as well.
// -> the hints in `out` and an empty string, or what is refused, "hint h: " + the condition, and `out` empty.  `modulus`: r, four words.
inline std::string decode_hints(const uint64_t *desc, size_t n_words, uint64_t ncols, const uint64_t *modulus, std::vector<Hint> &out) {
    out.clear();
    std::map<uint64_t, uint32_t> output_of;   // an output column -> the hint that names it
    size_t at = 0;
    std::string why;
    while (at < n_words && why.empty()) {
        const std::string here = "hint " + std::to_string(out.size()) + ": ";
        Hint h;
        h.index = (uint32_t)out.size();
        if (desc[at] != HINT_LONGDIV && desc[at] != HINT_MODDIV && desc[at] != HINT_LONGDIV_WIDE && desc[at] != HINT_MODMULDIV) { why = here + "unknown opcode " + std::to_string(desc[at]); break; }
        const bool moddiv = desc[at] == HINT_MODDIV;
        const bool muldiv = desc[at] == HINT_MODMULDIV;
        const size_t head = muldiv ? 13 : moddiv ? 9 : 7;
        if (n_words - at < head) { why = here + "the record is truncated"; break; }
        const uint64_t n = desc[at + 1], flags = desc[at + (muldiv ? 10 : head - 1)];
        if (n < 1 || n > HINT_MAX_N) { why = here + "n = " + std::to_string(n) + " is outside 1..128"; break; }
        uint64_t counts[4], kE;     // the lengths of q, rem, D, E; kE: the divisor's or the modulus' limbs, in columns or literal
        if (muldiv) {
            const uint64_t kz = desc[at + 2], kP = desc[at + 9], *k = desc + at + 3, cN = desc[at + 11], cD = desc[at + 12];   // k: kA, kB, kNp, kNm, kDp, kDm
            static const char *const names[MODMULDIV_LISTS] = {"kA", "kB", "kNp", "kNm", "kDp", "kDm"};
            if (kz < 1 || kz > MODDIV_MAX_KZ) { why = here + "kz = " + std::to_string(kz) + " is outside 1..16"; break; }
            for (uint32_t i = 0; i < MODMULDIV_LISTS && why.empty(); ++i)
                if (k[i] > MODDIV_MAX_K || (i < 2 && k[i] < 1)) why = here + names[i] + " = " + std::to_string(k[i]) + " is outside " + (i < 2 ? "1" : "0") + "..32";
            if (!why.empty()) break;
            if (k[5] > 0 && k[4] == 0) { why = here + "kDm = " + std::to_string(k[5]) + " with kDp = 0"; break; }
            if (kP < 1 || kP > MODDIV_MAX_KP) { why = here + "kP = " + std::to_string(kP) + " is outside 1..16"; break; }
            if (flags & ~HINT_MODULUS_LITERAL) { why = here + "unknown flags " + std::to_string(flags); break; }
            for (uint32_t i = 0; i < MODMULDIV_LISTS && why.empty(); ++i)
                if (k[i] && n * (k[i] - 1) >= MODDIV_OPERAND_BITS) why = here + "n (" + names[i] + " - 1) = " + std::to_string(n * (k[i] - 1)) + " is 1024 or more";
            if (!why.empty()) break;
            if (n * (kP - 1) >= MODDIV_MODULUS_BITS) { why = here + "n (kP - 1) = " + std::to_string(n * (kP - 1)) + " is 512 or more"; break; }
            if (cN < 1 || cN > MODMULDIV_MAX_C) { why = here + "cN = " + std::to_string(cN) + " is outside 1..4294967295"; break; }
            if (cD < 1 || cD > MODMULDIV_MAX_C) { why = here + "cD = " + std::to_string(cD) + " is outside 1..4294967295"; break; }
            h.op = (uint32_t)HINT_MODMULDIV;
            counts[0] = kz, counts[1] = 0, counts[2] = 0, kE = kP;
            for (uint32_t i = 0; i < MODMULDIV_LISTS; ++i) h.km[i] = (uint32_t)k[i], counts[2] += k[i];
            h.c[0] = (uint32_t)cN, h.c[1] = (uint32_t)cD;
        } else if (moddiv) {
            const uint64_t kz = desc[at + 2], kP = desc[at + 7], *k = desc + at + 3;   // k: kNp, kNm, kDp, kDm
            static const char *const names[4] = {"kNp", "kNm", "kDp", "kDm"};
            if (kz < 1 || kz > MODDIV_MAX_KZ) { why = here + "kz = " + std::to_string(kz) + " is outside 1..16"; break; }
            for (int i = 0; i < 4 && why.empty(); ++i)
                if (k[i] > MODDIV_MAX_K || (i == 2 && k[i] < 1)) why = here + names[i] + " = " + std::to_string(k[i]) + " is outside " + (i == 2 ? "1" : "0") + "..32";
            if (!why.empty()) break;
            if (kP < 1 || kP > MODDIV_MAX_KP) { why = here + "kP = " + std::to_string(kP) + " is outside 1..16"; break; }
            if (flags & ~HINT_MODULUS_LITERAL) { why = here + "unknown flags " + std::to_string(flags); break; }
            for (int i = 0; i < 4 && why.empty(); ++i)
                if (k[i] && n * (k[i] - 1) >= MODDIV_OPERAND_BITS) why = here + "n (" + names[i] + " - 1) = " + std::to_string(n * (k[i] - 1)) + " is 1024 or more";
            if (!why.empty()) break;
            if (n * (kP - 1) >= MODDIV_MODULUS_BITS) { why = here + "n (kP - 1) = " + std::to_string(n * (kP - 1)) + " is 512 or more"; break; }
            h.op = (uint32_t)HINT_MODDIV;
            for (int i = 0; i < 4; ++i) h.k[i] = (uint32_t)k[i];
            counts[0] = kz, counts[1] = 0, counts[2] = k[0] + k[1] + k[2] + k[3], kE = kP;
        } else if (desc[at] == HINT_LONGDIV_WIDE) {
            const uint64_t kq = desc[at + 2], kr = desc[at + 3], kD = desc[at + 4];
            kE = desc[at + 5];
            if (kq < 1 || kq > WIDE_MAX_KQ) { why = here + "kq = " + std::to_string(kq) + " is outside 1..128"; break; }
            if (kr < 1 || kr > WIDE_MAX_KR) { why = here + "kr = " + std::to_string(kr) + " is outside 1..64"; break; }
            if (kD < 1 || kD > WIDE_MAX_KD) { why = here + "kD = " + std::to_string(kD) + " is outside 1..128"; break; }
            if (kE < 1 || kE > WIDE_MAX_KE) { why = here + "kE = " + std::to_string(kE) + " is outside 1..64"; break; }
            if (flags & ~HINT_DIVISOR_LITERAL) { why = here + "unknown flags " + std::to_string(flags); break; }
            if (n * (kD - 1) >= WIDE_D_BITS) { why = here + "n (kD - 1) = " + std::to_string(n * (kD - 1)) + " is 8192 or more"; break; }
            if (n * (kE - 1) >= WIDE_E_BITS) { why = here + "n (kE - 1) = " + std::to_string(n * (kE - 1)) + " is 4096 or more"; break; }
            h.op = (uint32_t)HINT_LONGDIV_WIDE;
            counts[0] = kq, counts[1] = kr, counts[2] = kD;
        } else {
            const uint64_t kq = desc[at + 2], kr = desc[at + 3], kD = desc[at + 4];
            kE = desc[at + 5];
            if (kq < 1 || kq > HINT_MAX_KQ) { why = here + "kq = " + std::to_string(kq) + " is outside 1..32"; break; }
            if (kr < 1 || kr > HINT_MAX_KR) { why = here + "kr = " + std::to_string(kr) + " is outside 1..16"; break; }
            if (kD < 1 || kD > HINT_MAX_KD) { why = here + "kD = " + std::to_string(kD) + " is outside 1..32"; break; }
            if (kE < 1 || kE > HINT_MAX_KE) { why = here + "kE = " + std::to_string(kE) + " is outside 1..16"; break; }
            if (flags & ~HINT_DIVISOR_LITERAL) { why = here + "unknown flags " + std::to_string(flags); break; }
            if (n * (kD - 1) >= HINT_D_BITS) { why = here + "n (kD - 1) = " + std::to_string(n * (kD - 1)) + " is 1024 or more"; break; }
            if (n * (kE - 1) >= HINT_E_BITS) { why = here + "n (kE - 1) = " + std::to_string(n * (kE - 1)) + " is 512 or more"; break; }
            counts[0] = kq, counts[1] = kr, counts[2] = kD;
        }
        const bool literal = (flags & HINT_DIVISOR_LITERAL) != 0;   // HINT_MODULUS_LITERAL is the same bit
        counts[3] = literal ? 0 : kE;
        const uint64_t need = head + counts[0] + counts[1] + counts[2] + (literal ? 4 * kE : kE);
        if (n_words - at < need) { why = here + "the record is truncated"; break; }
        h.n = (uint32_t)n;
        h.flags = (uint32_t)flags;
        const uint64_t *w = desc + at + head;
        std::vector<uint32_t> *lists[4] = {&h.q, &h.rem, &h.D, &h.E};
        for (int l = 0; l < 4 && why.empty(); ++l)
            for (uint64_t i = 0; i < counts[l] && why.empty(); ++i, ++w) {
                if (*w >= ncols) why = here + "column " + std::to_string(*w) + " is not below m0 + mw = " + std::to_string(ncols);
                else lists[l]->push_back((uint32_t)*w);
            }
        if (!why.empty()) break;
        if (literal) {
            for (uint64_t i = 0; i < kE && why.empty(); ++i, w += 4)
                if (!words_less(w, modulus)) why = here + "literal limb " + std::to_string(i) + " is not below r";
                else h.lit.insert(h.lit.end(), w, w + 4);
            if (!why.empty()) break;
        }
        for (const std::vector<uint32_t> *outs : {&h.q, &h.rem})
            for (uint32_t col : *outs) {
                if (!why.empty()) break;
                if (col == 0) { why = here + "an output is column 0 (the constant one)"; break; }
                const auto named = output_of.find(col);
                if (named != output_of.end()) {
                    why = here + "output column " + std::to_string(col) + (named->second == h.index ? " is named twice" : " is an output of hint " + std::to_string(named->second) + " as well");
                    break;
                }
                output_of.emplace(col, h.index);
            }
        for (const std::vector<uint32_t> *in : {&h.D, &h.E})
            for (uint32_t col : *in) {
                const auto named = output_of.find(col);
                if (why.empty() && named != output_of.end() && named->second == h.index) why = here + "output column " + std::to_string(col) + " is an input of the hint as well";
            }
        if (!why.empty()) break;
        at += need;
        out.push_back(std::move(h));
    }
    if (!why.empty()) out.clear();
    return why;
}

// build_plan for rows in ANY order.  The matrix order is tried first: a system that build_plan accepts gets build_plan's plan,
// field for field, with reordered = false (and without the modulus, or with column 0 marked, there is nothing else).  Otherwise the
// scheduler above looks for a dependency order; if it finds one the plan has reordered = true, the same levels per column that the
// rows give in any solvable order, and the steps sorted by (level, kind, row) with the level_ptr and launches of finish_plan.  If it
// finds none the result is build_plan's error -- code, row, column, message -- with what stays unknown appended to the message.
// O(nnz log rows): a row is examined once, and once more per event on one of its unknown columns.
inline Plan build_plan_any_order(const Csr m[3], uint64_t nr, uint64_t m0, uint64_t mw, const uint8_t *unknown, uint32_t wide_steps = WIDE_STEPS,
                                 const uint64_t *modulus = nullptr, const std::vector<Hint> *hints = nullptr) {
    // the key's declared hints (decode_hints): active where every output carries the plain marker, inert where every output is given.
    // Without an active one everything below is what it was
    std::vector<Hint> active;
    const uint64_t ncols = m0 + mw;
    for (size_t h = 0; hints && modulus && h < hints->size() && !(ncols && unknown[0]); ++h) {
        size_t marked = 0, given = 0, special = 0;
        for (const std::vector<uint32_t> *outs : {&(*hints)[h].q, &(*hints)[h].rem})
            for (uint32_t col : *outs) (unknown[col] == PATTERN_UNKNOWN ? marked : unknown[col] ? special : given) += 1;
        if (special || (marked && given)) {
            Plan p;
            p.error = ERR_HINT;
            p.message = "hint " + std::to_string((*hints)[h].index) + ": " +
                        (special ? "an output carries the quotient, indicator or square-root marker" : "some outputs are marked unknown and some are given");
            return p;
        }
        if (marked) active.push_back((*hints)[h]);
    }
    if (!active.empty()) {   // the scheduler only: no row order solves a hint-owned column
        if (nr + hints->size() > 0xffffffffull) {
            Plan p;
            p.error = ERR_HINT;
            p.message = "rows and hints together exceed 2^32 - 1";
            return p;
        }
        Planner st(m, ncols, unknown, modulus);
        st.owned.assign(ncols, 0);
        for (const Hint &h : active)
            for (const std::vector<uint32_t> *outs : {&h.q, &h.rem})
                for (uint32_t col : *outs) st.owned[col] = 1;
        std::string why;
        if (!schedule_any_order(st, nr, ncols, why, &active)) {
            uint64_t col = 0;
            while (col < ncols && st.level[col] != Planner::UNSOLVED) ++col;
            st.fail(ERR_UNDETERMINED, 0, col < ncols ? col : 0, why);
            return std::move(st.p);
        }
        Plan &p = st.p;
        std::sort(p.steps.begin(), p.steps.end(), [](const Step &a, const Step &b) { return a.row < b.row; });   // a hint's row is nr + its index
        finish_plan(p, st.max_level, wide_steps);
        p.reordered = true;
        return std::move(p);
    }
    Plan first = build_plan(m, nr, m0, mw, unknown, wide_steps, modulus);
    if (first.error == OK || first.error == ERR_COLUMN_ZERO || !modulus) return first;
    Planner st(m, m0 + mw, unknown, modulus);
    std::string why;
    if (!schedule_any_order(st, nr, m0 + mw, why)) {
        first.message += "; in any row order: " + why;
        return first;
    }
    Plan &p = st.p;
    std::sort(p.steps.begin(), p.steps.end(), [](const Step &a, const Step &b) { return a.row < b.row; });   // a row gives at most one step
    finish_plan(p, st.max_level, wide_steps);
    p.reordered = true;
    return std::move(p);
}

}  // namespace pmsolve
