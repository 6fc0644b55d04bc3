"""The digit forms of a grouped call's scalars (hbbft_amd/csrc/group_digits.hpp, compiled with g++).

tests/csrc/group_digits_check.cpp replays the exact step sequence of the device's joint chains (start
value, doubling, table entry and its sign) over the integers mod r for every X4 tuple with digits in
{0, 1, 2^32 - 1}, every X2 tuple with digits in {0, 1, 2^64 - 1}, a single non-zero digit in each
position, leading-zero high digits and 10^4 random tuples, and compares with sum a_j |x|^j (X4, on the
two 32-step G2 chains and on the 96-step G1 chain of the halves a0 + a1 |x|, a2 + a3 |x|) and
b0 + b1 |x|^2 (X2, 64 steps); it checks that the zero residue is the all-zero tuple only (the one tuple a
grouped call rejects or redraws) and the coefficient bound behind the kernel's exceptional-addition
argument.  The same stand-alone program runs a second time built with the address and
undefined-behaviour sanitizers.

The claims of include/hbbft_hip.h are checked against the Python oracle: the two size bounds, and on
random subgroup points the identities the kernels rest on, with psi and beta restated from the curve's
constants."""
import os
import random
import re
import shutil
import subprocess

import pytest

from oracle import bls12_381 as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "csrc", "group_digits_check.cpp")
X = 0xd201000000010000  # |x|

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def _build(exe, extra):
    return subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", *extra, "-I",
                           os.path.join(ROOT, "hbbft_amd", "csrc"), "-o", exe, SRC], capture_output=True, text=True)


def _run(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"group_digits: 0 bad of (\d+)", out.stdout)
    assert m and int(m.group(1)) > 10 ** 6, out.stdout
    return out.stdout


@needs_gxx
def test_group_digits_chains(tmp_path):
    exe = str(tmp_path / "group_digits_check")
    b = _build(exe, [])
    assert b.returncode == 0, b.stderr
    _run(exe)


@needs_gxx
def test_group_digits_chains_sanitized(tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]
    p = subprocess.run(["g++", *san, "-o", str(tmp_path / "probe"), str(probe)], capture_output=True, text=True)
    if p.returncode != 0:
        pytest.skip("no sanitizer runtime for g++")
    exe = str(tmp_path / "group_digits_check_san")
    b = _build(exe, san)
    assert b.returncode == 0, b.stderr
    _run(exe)


def test_digit_forms_stay_below_r():
    assert X == C.X_ABS and C.R == X ** 4 - X ** 2 + 1
    top4 = (2 ** 32 - 1) * (1 + X + X ** 2 + X ** 3)
    top2 = (2 ** 64 - 1) * (1 + X ** 2)
    assert top4.bit_length() == 224 and top4 < C.R
    assert top2.bit_length() == 192 and top2 < C.R
    assert 2 ** 32 <= X and 2 ** 64 <= X ** 2  # digits below the base: the representation is unique
    assert (2 ** 32 - 1) * (1 + X) < 2 ** 96   # the G1 halves of X4


# psi and beta restated from the constants: xi = 1 + u, psi(x, y) = (conj(x) / xi^((p-1)/3), conj(y) / xi^((p-1)/2)),
# beta the cube root of unity with [x^2] (X, Y) = (beta X, -Y) on G1
XI = (1, 1)
PSI_CX = C.f2_inv(C.f2_pow(XI, (C.P - 1) // 3))
PSI_CY = C.f2_inv(C.f2_pow(XI, (C.P - 1) // 2))


def psi(q):
    return (C.f2_mul(C.f2_conj(q[0]), PSI_CX), C.f2_mul(C.f2_conj(q[1]), PSI_CY))


def beta_of_g1():
    """The cube root of unity beta with [x^2] P = (beta X, -Y), found from the generator."""
    gx, gy = C.G1_GEN
    px, py = C.g1_mul(C.G1_GEN, X * X % C.R)
    beta = px * C.fp_inv(gx) % C.P
    assert beta != 1 and pow(beta, 3, C.P) == 1 and py == (C.P - gy) % C.P
    return beta


def test_endomorphism_identities_on_random_points():
    rng = random.Random(2202)
    beta = beta_of_g1()
    for _ in range(3):
        q = C.g2_mul(C.G2_GEN, rng.randrange(1, C.R))
        p = C.g1_mul(C.G1_GEN, rng.randrange(1, C.R))
        assert psi(q) == C.g2_neg(C.g2_mul(q, X))  # psi = [x] = [-|x|] on G2
        p1, p2, p3 = psi(q), psi(psi(q)), psi(psi(psi(q)))
        # psi^2 scales x by an Fp constant (beta^2) and negates y; Q - psi^2 Q = -psi^4 Q = (beta x, -y)
        assert p2 == (C.f2_muls(q[0], beta * beta % C.P), C.f2_neg(q[1]))
        assert C.g2_add(q, C.g2_neg(p2)) == (C.f2_muls(q[0], beta), C.f2_neg(q[1]))
        lam = (beta * p[0] % C.P, (C.P - p[1]) % C.P)
        assert lam == C.g1_mul(p, X * X % C.R)
        assert C.g1_add(p, C.g1_neg(lam)) == (beta * beta * p[0] % C.P, (C.P - p[1]) % C.P)  # P - [x^2] P = -[x^4] P
        for a in ([rng.randrange(1 << 32) for _ in range(4)], [2 ** 32 - 1] * 4, [0, 1, 0, 2 ** 32 - 1]):
            r = sum(d * X ** j for j, d in enumerate(a))
            terms = [C.g2_mul(q, a[0]), C.g2_mul(C.g2_neg(p1), a[1]), C.g2_mul(p2, a[2]), C.g2_mul(C.g2_neg(p3), a[3])]
            acc = None
            for t in terms:
                acc = C.g2_add(acc, t)
            assert acc == C.g2_mul(q, r)
            assert C.g1_add(C.g1_mul(p, a[0] + a[1] * X), C.g1_mul(lam, a[2] + a[3] * X)) == C.g1_mul(p, r)
        for b in ([rng.randrange(1 << 64) for _ in range(2)], [2 ** 64 - 1] * 2):
            assert C.g1_add(C.g1_mul(p, b[0]), C.g1_mul(lam, b[1])) == C.g1_mul(p, b[0] + b[1] * X * X)


def test_header_macros_and_bound_symbols():
    from hbbft_amd import _lib
    from hbbft_amd.engine import Engine
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hbbft_hip.h")).read(), flags=re.S)
    m = {k: int(v, 0) for k, v in re.findall(r"^#define\s+(HBH_G[A-Z0-9_]+)\s+(-?\w+)\s*$", text, flags=re.M)}
    assert (m["HBH_GSCALAR_INT128"], m["HBH_GSCALAR_DIGITS"]) == (_lib.GSCALAR_INT128, _lib.GSCALAR_DIGITS) == (0, 1)
    assert (m["HBH_GFORM_INT128"], m["HBH_GFORM_X4"], m["HBH_GFORM_X2"]) == (_lib.GFORM_INT128, _lib.GFORM_X4,
                                                                             _lib.GFORM_X2) == (0, 1, 2)
    args = {s[0]: s[2] for s in _lib.SIGNATURES}
    assert len(args["hbh_engine_set_group_scalar_form"]) == 2   # (engine, form)
    assert len(args["hbh_dbg_group_sums_form"]) == 10           # hbh_dbg_group_sums' nine and the form
    assert len(args["hbh_dbg_group_sums"]) == 9
    assert callable(Engine.set_group_scalar_form) and callable(Engine.dbg_group_sums_form)


def test_batch_verifier_scalar_form_arguments():
    from hbbft_amd.protocol import BatchVerifier
    with pytest.raises(ValueError):
        BatchVerifier(None, scalar_form="digits")  # needs grouped=True
    with pytest.raises(ValueError):
        BatchVerifier(None, grouped=True, scalar_form="x4")
    assert BatchVerifier(None, grouped=True).scalar_form == "int128"
    assert BatchVerifier(None, grouped=True, scalar_form="digits").scalar_form == "digits"
    assert BatchVerifier(None).scalar_form is None


def test_digit_scalar_packing():
    from hbbft_amd import _lib
    from hbbft_amd.engine import digit_scalar
    packed, value = digit_scalar(_lib.GFORM_X4, [1, 2, 3, 4])
    assert packed.to_bytes(16, "little") == b"".join(d.to_bytes(4, "little") for d in (1, 2, 3, 4))
    assert value == 1 + 2 * X + 3 * X ** 2 + 4 * X ** 3
    packed, value = digit_scalar(_lib.GFORM_X2, [5, 2 ** 64 - 1])
    assert packed.to_bytes(16, "little") == (5).to_bytes(8, "little") + b"\xff" * 8
    assert value == 5 + (2 ** 64 - 1) * X * X
    with pytest.raises(ValueError):
        digit_scalar(_lib.GFORM_X4, [1, 2, 3])
    with pytest.raises(ValueError):
        digit_scalar(_lib.GFORM_X2, [1, 2 ** 64])


def test_workcount_digit_forms():
    from hbbft_amd import workcount as W
    for kind, form, ratio in (("g2", "x4", 0.5), ("g1", "x4", 0.75), ("g1", "x2", 0.5)):
        tree = W.group_sum_critical_path(kind, "chain", 64) - (128 if kind == "g1" else 64) * sum(W.GSUM_OPS[kind][:2])
        digits = W.group_sum_critical_path(kind, form, 64)
        chain = W.group_sum_critical_path(kind, "chain", 64)
        assert digits < chain
        # the chain part shortens in proportion to the steps
        steps = W.GSUM_DIGIT_CHAINS[(kind, form)][1]
        assert steps == ratio * (128 if kind == "g1" else 64)
        assert W.group_sum_ops(kind, form, 64) < W.group_sum_ops(kind, "chain", 64)
        assert tree > 0
    with pytest.raises(ValueError):
        W.group_sum_ops("g2", "x2", 64)
