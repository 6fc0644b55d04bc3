"""Algorithmic work of the hot-path units, in Fp multiplications, derived from the kernels' own
formulas (csrc/pfp.hpp, k_pair.hip, curve.hpp).  Used by bench.py for the roofline's 'achieved'
figure.  Fp2 mul = 3 Fp-mul (Karatsuba), Fp2 sqr = 2 (complex), Fp2 x Fp = 2.

Pricing: one Fp multiplication = 300 32x32->64 multiply-adds (12-limb CIOS
Montgomery: 144 product + 156 reduction); an Fp squaring = 222 (78 product + 144 reduction).
True Fp squarings occur in the Fp inversion (380 of them) and in the G1 curve formulas
(dbl-2009-l 2M+5S, madd-2007-bl 7M+4S, add-2007-bl 11M+5S); Fp2/Fp12 squarings are products.
"""
X_ABS = 0xD201000000010000
NBITS = X_ABS.bit_length() - 1          # 63 doubling steps
NADD = bin(X_ABS).count("1") - 1        # 5 addition steps
F2M, F2S, F2F = 3, 2, 2

F6_MUL = 6 * F2M                         # 18
F12_SQR = 2 * F6_MUL                     # 36 (complex squaring)
F12_MUL = 3 * F6_MUL                     # 54
F12_MUL_014 = 2 * 5 * F2M + 3 * F2M      # 39
LINE_EVAL = 2 * F2F                      # c1*xP, c4*yP
CYCLO_SQR = 9 * F2S                      # 18 (Granger-Scott)
FROB1 = 5 * F2M
FROB2 = 5 * F2F

DBL_STEP = 7 * F2S + 4 * F2M             # 26
ADD_STEP = 3 * F2S + 10 * F2M            # 36
G2_WALK = NBITS * DBL_STEP + NADD * ADD_STEP

MILLER_2PAIR = NBITS * (F12_SQR + 2 * (F12_MUL_014 + LINE_EVAL)) + NADD * 2 * (F12_MUL_014 + LINE_EVAL)

# The final exponentiation's one Fp inversion (of a public norm) is T. Pornin's binary GCD
# (words.hpp words_inv_vartime): 25 rounds of 31 divsteps on 64-bit approximations; per round the
# 2x2 update of (a, b) (2 x 12 limbs x 2 MADs each) and of the Bezout pair (u, v) with its
# Montgomery division by 2^31 (2 x (24 + 12) MADs) = 120 MADs -> 3,000 MADs = 10 Fp products.
# (Round 2 priced Fermat's a^(p-2): 380 squarings + 190 products.)
BINGCD_ROUNDS = (2 * 381 - 1 + 30) // 31
BINGCD_MADS = BINGCD_ROUNDS * 120
FP_INV = BINGCD_MADS // 300
F2_INV = 2 + FP_INV + 2
F6_INV = 3 * (F2S + F2M) + 3 * F2M + F2_INV + 3 * F2M
F12_INV = 2 * F6_MUL + F6_INV + 2 * F6_MUL
EASY = F12_INV + F12_MUL + FROB2 + F12_MUL


def _exp(e):
    return NBITS * CYCLO_SQR + (bin(e).count("1") - 1) * F12_MUL


HARD = 2 * _exp(X_ABS + 1) + 3 * _exp(X_ABS) + FROB1 + FROB2 + 5 * F12_MUL + CYCLO_SQR
FINAL_EXP = EASY + HARD

# per check: multi-Miller loop over (pk_i, H) and (-g1, sig_i), the G2 walk over sig_i (H's walk
# is shared by the 64 shares of a document), one final exponentiation
FP_MULS_PER_CHECK = MILLER_2PAIR + G2_WALK + FINAL_EXP

# The reference's work for the same verdict (SURVEY §8(d) "reference work"): threshold_crypto's
# verify_g2 computes e(pk_i, H) and e(g1, sig_i) as two separate pairings (pairing 0.14: each its own
# G2Prepared walk, single-pair Miller loop and final exponentiation), then compares them.
MILLER_1PAIR = NBITS * (F12_SQR + F12_MUL_014 + LINE_EVAL) + NADD * (F12_MUL_014 + LINE_EVAL)
REFERENCE_CHECK = 2 * (MILLER_1PAIR + G2_WALK + FINAL_EXP)

if __name__ == "__main__":
    print("miller", MILLER_2PAIR, "g2 walk", G2_WALK, "final exp", FINAL_EXP, "(easy", EASY, "hard", HARD,
          ") total", FP_MULS_PER_CHECK)


# ---------------------------------------------------------------------------- MAD pricing
MAD_PER_FPMUL = 300
MAD_PER_FPSQR = 222
FP_INV_SQR = 0                        # binary-GCD inverse: no Fp squarings (Fermat had 380)


def mads(fpmul, fpsqr=0):
    """32x32->64 multiply-adds of fpmul products (of which fpsqr are squarings)."""
    return (fpmul - fpsqr) * MAD_PER_FPMUL + fpsqr * MAD_PER_FPSQR


# per-unit algorithmic work of each kernel: (Fp ops, of which Fp squarings)
PAIR_CHECK_WALK = (MILLER_2PAIR + G2_WALK + FINAL_EXP, FP_INV_SQR)   # k_pair_verify, one side walked
PAIR_CHECK_TABLE = (MILLER_2PAIR + FINAL_EXP, FP_INV_SQR)            # k_pair_verify, both sides tabled
PAIR_PREP_DOC = (G2_WALK, 0)                                         # k_oct_prep, per G2 point
REFERENCE_CHECK_OPS = (REFERENCE_CHECK, FP_INV_SQR)                  # two separate pairings

G1_DBL = (7, 5)
G1_MADD = (11, 4)
G1_ADD = (16, 5)


def _add(*ops):
    return (sum(o[0] for o in ops), sum(o[1] for o in ops))


def _scale(op, k):
    return (op[0] * k, op[1] * k)


def g1_mul_small(k):
    """jac_mul_small(P, k): double-and-add from the top bit with full Jacobian additions."""
    if k <= 1:
        return (0, 0)
    return _add(_scale(G1_DBL, k.bit_length() - 1), _scale(G1_ADD, bin(k).count("1") - 1))


def bivar_ack(t, y, val_windows=32):
    """k_bivar_check for one ack: Horner over the t+1 row points with the small y, then g1 * val
    from the fixed-base comb table (one mixed addition per nonzero byte of val: 32 windows) and a
    cross-multiplied compare."""
    horner = _scale(_add(g1_mul_small(y), G1_MADD), t + 1)
    return _add(horner, _scale(G1_MADD, val_windows), (4, 2))


def bivar_row_fd(t, ymin, ymax, nacks, val_windows=16):
    """The finite-difference Ack check of one row (k_bivar_fd_seed / _run / _check): the difference
    table at y0 (0 when ymin <= t + 1, as the engine's plan_fd seeds) by the seed levels -- per level
    m < t and k = 1 .. t - m one product k (D_k + D_{k-1}) for y0 = 0, else (y0 + k) D_k + k D_{k-1},
    and per level one mixed addition of R_m --, t additions per further y (ymax - y0 steps), and per
    ack g1 * val from the 16-bit comb (one mixed addition per nonzero 16-bit window) and the compare."""
    y0 = 0 if ymin <= t + 1 else ymin
    parts = [_scale(G1_MADD, t + 1)]
    for m in range(t - 1, -1, -1):
        for k in range(1, t - m + 1):
            if y0 == 0:
                parts.append(_add(G1_ADD, g1_mul_small(k)))
            else:
                parts.append(_add(G1_ADD, g1_mul_small(y0 + k), g1_mul_small(k)))
    steps = _scale(G1_ADD, t * (ymax - y0))
    acks = _scale(_add(_scale(G1_MADD, val_windows), (4, 2)), nacks)
    return _add(*parts, steps, acks)


# ---------------------------------------------------------------------------- wire decoding (round 6)
# k_g1_decompress / k_g2_decompress per valid point (csrc/k_wire.hip).  The square root's one
# exponent (p-3)/4 is tools/gen_sqrt_chain.py's width-4 sliding-window chain: a^2 + 375 squarings
# and 7 table + 78 window products.
SQRT_CHAIN = (376 + 85, 376)
G2_DBL = (2 * F2M + 5 * F2S, 0)          # dbl-2009-l over Fp2 (Fp2 squarings are Fp products)
G2_MADD = (7 * F2M + 4 * F2S, 0)         # madd-2007-bl over Fp2
# G1: to Montgomery, x^3 + 4, y = rhs * rhs^((p-3)/4) and its check, canonical y; subgroup by
# phi(P') == [-x^2] P' on the isomorphic point P' = (rhs x, rhs^2) (2 products): [|x|] twice (63
# doublings + 5 mixed / 5 general additions), beta x and the Jacobian-affine compare.  (One chain over
# x^2 -- 127 doublings + 16 mixed additions -- spills less but measured slower: 2.09 vs 1.96 ms.)
WIRE_G1_DECODE = _add((1, 0), (2, 1), SQRT_CHAIN, (2, 1), (1, 0), (2, 1),
                      _scale(G1_DBL, 2 * NBITS), _scale(G1_MADD, NADD), _scale(G1_ADD, NADD), (5, 1))
# G2: to Montgomery, x^3 + b, the norm-method root (norm, two chains, s, t, t w, a1 w / 2, t w^2,
# the y^2 check), the sign's canonical compare; subgroup by psi(P) == [x] P: [|x|] (63 doublings +
# 5 mixed additions), psi and the compare
WIRE_G2_DECODE = _add((2, 0), (F2S + F2M, 0), (2, 2), _scale(SQRT_CHAIN, 2), (1, 0), (1, 1), (1, 0),
                      (1, 0), (2, 0), (1, 0), (F2S, 0), (6, 0),
                      _scale(G2_DBL, NBITS), _scale(G2_MADD, NADD), (2 + F2M, 0), (F2S + 3 * F2M, 0))


# ---------------------------------------------------------------------------- wire decoding, per role
# Both decoder forms run two roles side by side in one workgroup, so a small batch takes the longer
# role's serial chain.  Critical paths below are in Fp-product times: one lane's Fp product = 1, a
# round of lane-quad products = 1 (g1quad.hpp: every lane forms one Fp product), a round of
# lane-pair products = 1.5 (pfp.hpp h_mul: 588 multiply-adds per lane against 392 for an Fp product).
WIRE_ROOT_G1 = 1 + 2 + SQRT_CHAIN[0] + 2 + 1            # to Montgomery, x^3 + 4, chain, y and its check, canonical y
WIRE_ROOT_G2 = (2 + (F2S + F2M) + 2 + 2 * SQRT_CHAIN[0]  # to Montgomery, x^3 + b, norm, two dependent chains,
                + 1 + 1 + 1 + 1 + 2 + 1 + F2S + 6 + 2)  # s, s^2, t, t w, a1 w / 2, t w^2, y^2, sign compare, N(y)
# HBH_DEC_LANE (k_wire.hip): one lane runs the whole [|x|] chain(s)
WIRE_LANE_SUB_G1 = 1 + 2 + 2 + 2 * NBITS * G1_DBL[0] + NADD * (G1_MADD[0] + G1_ADD[0]) + 5
WIRE_LANE_SUB_G2 = (2 + (F2S + F2M) + (F2S + F2M) + NBITS * G2_DBL[0] + NADD * G2_MADD[0]
                    + (2 + F2M) + (F2S + 3 * F2M) + 2)
# HBH_DEC_SPLIT (k_wire_split.hip): product rounds of the lane-quad group law
G1Q_DBL_ROUNDS, G1Q_MADD_ROUNDS, G1Q_ADD_ROUNDS = 3, 5, 5     # g1quad.hpp
G2Q_DBL_ROUNDS, G2Q_MADD_ROUNDS = 4, 6                        # g2quad.hpp
LANE_PAIR_PRODUCT = 1.5
WIRE_SPLIT_SUB_G1_ROUNDS = (1 + 2 + 1 + 2 * NBITS * G1Q_DBL_ROUNDS + NADD * (G1Q_MADD_ROUNDS + G1Q_ADD_ROUNDS)
                            + 3)                              # ... P' in one round, the compare in three
WIRE_SPLIT_SUB_G2_ROUNDS = 2 + 1 + NBITS * G2Q_DBL_ROUNDS + NADD * G2Q_MADD_ROUNDS + 4   # lane-pair rounds
WIRE_SPLIT_SUB_G2_FP = 1 + 1 + 1                              # to Montgomery, C1 conj(x), the factor N(y)

WIRE_DECODE_ROLES = {
    # (group, form): critical path of each role, Fp-product times
    ("g1", "lane"): {"root": WIRE_ROOT_G1, "subgroup": WIRE_LANE_SUB_G1},
    ("g2", "lane"): {"root": WIRE_ROOT_G2, "subgroup": WIRE_LANE_SUB_G2},
    ("g1", "split"): {"root": WIRE_ROOT_G1, "subgroup": WIRE_SPLIT_SUB_G1_ROUNDS},
    ("g2", "split"): {"root": WIRE_ROOT_G2,
                      "subgroup": WIRE_SPLIT_SUB_G2_ROUNDS * LANE_PAIR_PRODUCT + WIRE_SPLIT_SUB_G2_FP},
}
# products issued per point (every lane of a quad forms a product in every round)
WIRE_DECODE_PRODUCTS = {
    ("g1", "lane"): WIRE_ROOT_G1 + WIRE_LANE_SUB_G1,
    ("g2", "lane"): WIRE_ROOT_G2 + WIRE_LANE_SUB_G2,
    ("g1", "split"): WIRE_ROOT_G1 + 4 * WIRE_SPLIT_SUB_G1_ROUNDS,
    ("g2", "split"): WIRE_ROOT_G2 + 4 * (WIRE_SPLIT_SUB_G2_ROUNDS * LANE_PAIR_PRODUCT + WIRE_SPLIT_SUB_G2_FP),
}


def wire_decode_critical_path(group, form):
    """The longer role's chain: what a batch small enough to give every wave its own SIMD waits for."""
    return max(WIRE_DECODE_ROLES[(group, form)].values())


def wire_split_model_ratio(group):
    """Predicted SPLIT / LANE time of a small batch (op model only: no issue rate, no memory)."""
    return wire_decode_critical_path(group, "split") / wire_decode_critical_path(group, "lane")


# ---------------------------------------------------------------------------- group sums (grouped share checks)
# One tile of L items of the sums sum_i r_i P_i (r_i: 128 unstructured random bits), per form
# (hbh_engine_set_group_sum_impl), in Fp products from the per-operation weights above.
G2_ADD = (11 * F2M + 5 * F2S, 0)         # add-2007-bl over Fp2
GSUM_OPS = {"g1": (G1_DBL[0], G1_MADD[0], G1_ADD[0]), "g2": (G2_DBL[0], G2_MADD[0], G2_ADD[0])}
GSUM_WINDOWS = {"g1": 64, "g2": 32}      # two-bit windows: 128 bits of r (G1), d0 and d1 < |x| < 2^64 (G2)
GSUM_TAIL_SEGS = 8                       # csrc/group_bucket.hpp TAIL_SEGS
GSUM_D2_RATE = 1.0 - (X_ABS * X_ABS) / 2.0 ** 128   # share of the scalars >= |x|^2: the psi^2(P) term
# The digit forms of the scalars (hbh_engine_set_group_scalar_form, csrc/group_digits.hpp): joint chains of
# two digits, (chains per item, steps per chain) by (kind, form); a step adds unless both digit bits are 0.
GSUM_DIGIT_CHAINS = {("g1", "x4"): (1, 96), ("g1", "x2"): (1, 64), ("g2", "x4"): (2, 32)}
GSUM_DIGIT_ADD_RATE = 0.75


def _gsum_tail(kind):
    """(doublings, additions) of the bucket form's tail and the same for its longest lane: TAIL_SEGS
    Horner runs of windows / TAIL_SEGS windows, each shifted by its weight, then a tree."""
    seg = GSUM_WINDOWS[kind] // GSUM_TAIL_SEGS
    dbl = sum(2 * (seg - 1) + 2 * seg * s for s in range(GSUM_TAIL_SEGS))
    add = GSUM_TAIL_SEGS * (seg - 1) + GSUM_TAIL_SEGS - 1
    path = (2 * (seg - 1) + 2 * seg * (GSUM_TAIL_SEGS - 1), (seg - 1) + GSUM_TAIL_SEGS.bit_length() - 1)
    return (dbl, add), path


def group_sum_ops(kind, impl, L):
    """Fp products issued for one tile of L items ("g1" / "g2", "chain" / "bucket"), expected over
    random scalars.
      chain (k_group_sum): one double-and-add chain per (item, digit): G1 128 doublings and 64 mixed
        additions per item; G2 two chains of 64 and 32, the psi^2(P) addition for r >= |x|^2 and the
        addition of the second chain into the first; then L - 1 additions of the tree.
      bucket (k_group_bucket): 3/4 of the (term, window) digits are nonzero, one mixed addition each
        (G1: L terms x 64 windows; G2: 2 L terms x 32 windows, plus the psi^2(P) terms in window 0);
        3 additions and a doubling per window to reduce the buckets; the tail.
      x4 / x2 (k_group_digits, the digit forms): one joint chain per pair of digits, a doubling per step
        and a mixed addition at 3/4 of the steps (G1: 96 steps under x4, 64 under x2; G2, x4 only: two
        chains of 32, the second added into the first), two Fp products per Fp coordinate for the scaled
        abscissae of a chain's table; then the tree."""
    dbl, madd, add = GSUM_OPS[kind]
    if (kind, impl) in GSUM_DIGIT_CHAINS:
        chains, steps = GSUM_DIGIT_CHAINS[(kind, impl)]
        table = 2 if kind == "g1" else 4
        per_chain = steps * (dbl + GSUM_DIGIT_ADD_RATE * madd) + table
        return L * chains * per_chain + L * (chains - 1) * add + (L - 1) * add
    if impl == "chain":
        if kind == "g1":
            return L * (128 * dbl + 64 * madd) + (L - 1) * add
        return 2 * L * (64 * dbl + 32 * madd) + L * GSUM_D2_RATE * madd + L * add + (L - 1) * add
    if impl != "bucket":
        raise ValueError(impl)
    nw = GSUM_WINDOWS[kind]
    terms = L if kind == "g1" else 2 * L
    acc = 0.75 * terms * nw * madd + (L * GSUM_D2_RATE * madd if kind == "g2" else 0)
    (tdbl, tadd), _ = _gsum_tail(kind)
    return acc + nw * (3 * add + dbl) + tdbl * dbl + tadd * add


def group_sum_critical_path(kind, impl, L):
    """Fp-product times of the longest lane of one tile's workgroup.  Under SIMT a lane executes a
    masked addition whenever any lane of its wave takes it, so a chain pays the addition at every bit
    and a bucket lane at every term.  A digit form's joint chain pays it at every step the same way."""
    dbl, madd, add = GSUM_OPS[kind]
    if (kind, impl) in GSUM_DIGIT_CHAINS:
        chains, steps = GSUM_DIGIT_CHAINS[(kind, impl)]
        width = 64
        while width < L:
            width *= 2
        return steps * (dbl + madd) + (chains - 1) * add + (width.bit_length() - 1) * add
    if impl == "chain":
        width = 64
        while width < L:
            width *= 2
        tree = (width.bit_length() - 1) * add
        if kind == "g1":
            return 128 * (dbl + madd) + tree
        return 64 * (dbl + madd) + madd + add + tree
    if impl != "bucket":
        raise ValueError(impl)
    _, (pdbl, padd) = _gsum_tail(kind)
    slots = L if kind == "g1" else 2 * L + L * GSUM_D2_RATE   # window 0's wave takes the psi^2(P) terms
    return slots * madd + (3 * add + dbl) + pdbl * dbl + padd * add


# ---------------------------------------------------------------------------- batched independent checks
# hbh_verify_signatures_batched / hbh_verify_ciphertexts_uv_batched against the per-item check, per ITEM,
# in Fp products from the weights above.  An op model only: what the calls measure is profiles/r25.
BATCH_GROUP = 256                         # HBH_BATCH_GROUP: items per final exponentiation
BATCH_TILE_ITEMS = {2: 256, 4: 128, 8: 64}   # items per workgroup of the Miller-product kernel, by lanes per slot
PER_ITEM_CHECK = MILLER_2PAIR + 2 * G2_WALK + FINAL_EXP   # the unbatched call: both sides walked
# an item is ONE side of a two-item slot: half a 2-pair Miller loop and one walk
BATCH_MILLER_ITEM = MILLER_2PAIR / 2 + G2_WALK
# r_i P_i: the X4 joint chain of 96 steps with one lane per item -- under SIMT every lane pays every
# addition --, the two scaled abscissae of its table, and the affine output (an inversion, Z^-2, Z^-3, x, y)
BATCH_G1_CHAIN = 96 * (G1_DBL[0] + G1_MADD[0]) + 2 + (FP_INV + 5)
# the item's share of sum r_i B_i in G2: two joint chains of 32 steps (every lane pays every addition), their
# tables, the second chain added into the first, and one addition of the tile's tree
BATCH_G2_SUM_ITEM = 2 * (32 * (G2_DBL[0] + G2_MADD[0]) + 4) + 2 * G2_ADD[0]
# per group: the closing pair (one Miller-only wave check), one final exponentiation
BATCH_CLOSING_GROUP = MILLER_1PAIR + G2_WALK


def batch_tree_item(lanes, executed=True):
    """The Fp12 products of the product tree, per item.  Issued: a tile of T items multiplies T / 2 slot
    values with T / 2 - 1 products, and the wave kernel's product mode multiplies the group's tiles and the
    closing value -- 128 products per 256 items at every width.  Executed: a wave runs a level's product
    whenever one of its slots multiplies, so every slot pays log2(T / 2) products (the default)."""
    slots = BATCH_TILE_ITEMS[lanes] // 2
    tpg = BATCH_GROUP // BATCH_TILE_ITEMS[lanes]
    if executed:
        return ((slots.bit_length() - 1) * F12_MUL) / 2 + tpg * F12_MUL / BATCH_GROUP
    return ((slots - 1) * tpg + tpg) * F12_MUL / BATCH_GROUP


def batched_model(lanes=2, executed=True):
    """Per-item entries of the batched check with no failed group: {entry: Fp products}."""
    return {
        "miller_product": BATCH_MILLER_ITEM,
        "tree": batch_tree_item(lanes, executed),
        "g1_chain": BATCH_G1_CHAIN,
        "g2_sum": BATCH_G2_SUM_ITEM,
        "closing_pair": BATCH_CLOSING_GROUP / BATCH_GROUP,
        "final_exp": FINAL_EXP / BATCH_GROUP,
    }


def batched_model_ratio(lanes=2, executed=True, pairing_only=False):
    """Model cost of the batched check over the per-item check (no failed group; a failed group pays
    both).  pairing_only: HBH_STAGE_PAIRING's entries against the same per-item check."""
    m = batched_model(lanes, executed)
    if pairing_only:
        m = {k: v for k, v in m.items() if k not in ("g1_chain", "g2_sum")}
    return sum(m.values()) / PER_ITEM_CHECK
