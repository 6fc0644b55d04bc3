"""The trial messages of the device-hash tests: b"hbh-trial-%d" needs between 1 and 12 candidate x before one
gives a square, counted here with the oracle's stream.  No GPU and no torch: importable by any test."""
from oracle import bls12_381 as C
from oracle import tc


def trial(i):
    return b"hbh-trial-%d" % i


def candidates(msg):
    """how many x G2::rand draws for msg before x^3 + b is a square: a in Fq2 is a square iff its norm
    is a square in Fq"""
    rng = tc.ChaChaRng(tc.sha3_256(msg))
    k = 0
    while True:
        k += 1
        x = (rng.gen_fq(), rng.gen_fq())
        rng.gen_bool()
        a = C.f2_add(C.f2_mul(C.f2_sqr(x), x), C.B2)
        nrm = (a[0] * a[0] + a[1] * a[1]) % C.P
        if nrm == 0 or pow(nrm, (C.P - 1) // 2, C.P) == 1:
            return k
