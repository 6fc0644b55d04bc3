"""ctypes binding of the C ABI in include/hbbft_hip.h (libhbbft_hip.so, built in-tree).

Loading fails loudly when the shared library is missing: there is no CPU fallback anywhere in
the product path.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# HBBFT_HIP_LIB overrides the in-tree library (A/B builds of the same sources)
LIB_PATH = os.environ.get("HBBFT_HIP_LIB") or os.path.join(_HERE, "libhbbft_hip.so")

G1_BYTES = 96
G2_BYTES = 192
FR_BYTES = 32

# (name, restype, argtypes) for every symbol declared in include/hbbft_hip.h
_c = ctypes
_P = _c.c_void_p
_SZ = _c.c_size_t
_I = _c.c_int
SIGNATURES = [
    ("hbh_engine_create", _I, [_I, _c.POINTER(_P)]),
    ("hbh_engine_destroy", _I, [_P]),
    ("hbh_last_error", _c.c_char_p, []),
    ("hbh_device_count", _I, [_c.POINTER(_I)]),
    ("hbh_verify_pairing_eq", _I, [_P, _SZ, _P, _P, _SZ, _P, _P, _P, _SZ, _P, _P]),
    ("hbh_verify_sig_shares", _I, [_P, _SZ, _P, _P, _P, _SZ, _P, _P]),
    ("hbh_verify_dec_shares", _I, [_P, _SZ, _P, _P, _P, _P, _SZ, _P, _P]),
    ("hbh_verify_ciphertexts", _I, [_P, _SZ, _P, _P, _P, _P]),
    # grouped random-combination share checks (opt-in)
    ("hbh_verify_sig_shares_grouped", _I, [_P, _SZ, _P, _P, _P, _SZ, _P, _P, _P, _P]),
    ("hbh_verify_dec_shares_grouped", _I, [_P, _SZ, _P, _P, _P, _P, _SZ, _P, _P, _P, _P]),
    ("hbh_dbg_group_sums", _I, [_P, _SZ, _P, _P, _SZ, _P, _P, _P, _P]),
    ("hbh_engine_set_group_sum_impl", _I, [_P, _I]),
    ("hbh_engine_set_group_scalar_form", _I, [_P, _I]),
    ("hbh_dbg_group_sums_form", _I, [_P, _I, _SZ, _P, _P, _SZ, _P, _P, _P, _P]),
    ("hbh_verify_pairing_eq_dev", _I, [_P, _P, _SZ, _P, _P, _SZ, _P, _P, _P, _SZ, _P, _P]),
    ("hbh_dbg_pairing", _I, [_P, _SZ, _P, _P, _P]),
    ("hbh_interpolate_g2", _I, [_P, _SZ, _I, _P, _P, _P, _P]),
    ("hbh_interpolate_g1", _I, [_P, _SZ, _I, _P, _P, _P, _P]),
    ("hbh_combine_verify_g2", _I, [_P, _SZ, _I, _P, _P, _P, _P, _P, _P, _P]),
    ("hbh_g1_mul", _I, [_P, _SZ, _P, _P, _P]),
    ("hbh_g2_mul", _I, [_P, _SZ, _P, _P, _P]),
    ("hbh_g1_mul_gen", _I, [_P, _SZ, _P, _P]),
    ("hbh_bivar_row", _I, [_P, _SZ, _I, _SZ, _P, _P, _P, _P]),
    ("hbh_g1_decompress", _I, [_P, _SZ, _P, _P, _P]),
    ("hbh_g2_decompress", _I, [_P, _SZ, _P, _P, _P]),
    ("hbh_commitment_eval", _I, [_P, _SZ, _I, _SZ, _P, _P, _P, _P]),
    ("hbh_bivar_ack_check", _I, [_P, _SZ, _I, _SZ, _P, _P, _P, _P, _P, _P]),
    ("hbh_commit_set_create", _I, [_P, _I, _c.POINTER(_P)]),
    ("hbh_commit_set_destroy", _I, [_P]),
    ("hbh_commit_set_add", _I, [_P, _SZ, _P, _c.POINTER(_SZ)]),
    ("hbh_commit_set_size", _I, [_P, _c.POINTER(_SZ), _c.POINTER(_SZ)]),
    ("hbh_bivar_row_set", _I, [_P, _SZ, _P, _P, _P]),
    ("hbh_bivar_ack_check_set", _I, [_P, _SZ, _P, _P, _P, _P, _P]),
    # device-resident prepared G2 points
    ("hbh_g2_set_create", _I, [_P, _SZ, _c.POINTER(_P)]),
    ("hbh_g2_set_destroy", _I, [_P]),
    ("hbh_g2_set_add", _I, [_P, _SZ, _P, _P]),
    ("hbh_g2_set_release", _I, [_P, _SZ, _P]),
    ("hbh_g2_set_size", _I, [_P, _c.POINTER(_SZ), _c.POINTER(_SZ)]),
    ("hbh_verify_pairing_eq_set", _I, [_P, _SZ, _P, _P, _P, _SZ, _P, _P, _P, _P, _SZ, _P, _P]),
    ("hbh_verify_sig_shares_set", _I, [_P, _SZ, _P, _P, _P, _P, _P]),
    ("hbh_verify_dec_shares_set", _I, [_P, _SZ, _P, _P, _P, _P, _P, _P]),
    ("hbh_verify_pairing_eq_set_dev", _I, [_P, _P, _SZ, _P, _P, _P, _SZ, _P, _P, _P, _P, _SZ, _P, _P]),
    ("hbh_engine_set_pairing_impl", _I, [_P, _I]),
    ("hbh_engine_set_ack_impl", _I, [_P, _I]),
    ("hbh_engine_set_decode_impl", _I, [_P, _I]),
    ("hbh_engine_set_hash_impl", _I, [_P, _I]),
    ("hbh_engine_set_hash_form", _I, [_P, _I]),
    ("hbh_dbg_set_hash_rounds", _I, [_P, _I]),
    # hashing to G2 on the device
    ("hbh_engine_hash_g2", _I, [_P, _SZ, _P, _P, _P]),
    ("hbh_engine_hash_g1_g2", _I, [_P, _SZ, _P, _P, _P, _P]),
    ("hbh_hash_g2_dev", _I, [_P, _P, _SZ, _P, _P]),
    ("hbh_verify_signatures", _I, [_P, _SZ, _P, _P, _P, _P, _P]),
    ("hbh_engine_hash_g1_g2_bp", _I, [_P, _SZ, _P, _P, _P, _P]),
    ("hbh_verify_ciphertexts_uv", _I, [_P, _SZ, _P, _P, _P, _P, _P]),
    ("hbh_engine_encrypt", _I, [_P, _SZ, _P, _I, _P, _P, _P, _P, _P, _P]),
    # batched independent checks (opt-in): one final exponentiation per BATCH_GROUP items
    ("hbh_verify_signatures_batched", _I, [_P, _SZ, _P, _P, _P, _P, _P, _P, _P]),
    ("hbh_verify_ciphertexts_uv_batched", _I, [_P, _SZ, _P, _P, _P, _P, _P, _P, _P]),
    ("hbh_dbg_pairing_product", _I, [_P, _SZ, _P, _P, _P]),
    ("hbh_engine_set_profiling", _I, [_P, _I]),
    ("hbh_engine_stage_time", _I, [_P, _I, _c.POINTER(_c.c_double), _c.POINTER(_I)]),
    # device-resident variants
    ("hbh_interpolate_g1_dev", _I, [_P, _P, _SZ, _I, _P, _P, _P, _P]),
    ("hbh_interpolate_g2_dev", _I, [_P, _P, _SZ, _I, _P, _P, _P, _P]),
    ("hbh_g1_decompress_dev", _I, [_P, _P, _SZ, _P, _P, _P]),
    ("hbh_g2_decompress_dev", _I, [_P, _P, _SZ, _P, _P, _P]),
    ("hbh_bivar_ack_check_dev", _I, [_P, _P, _SZ, _I, _P, _SZ, _P, _P, _P, _P, _P, _P]),
    # engine pool (multi-device fan-out)
    ("hbh_pool_create", _I, [_P, _I, _c.POINTER(_P)]),
    ("hbh_pool_destroy", _I, [_P]),
    ("hbh_pool_shards", _I, [_P, _c.POINTER(_I)]),
    ("hbh_pool_engine", _I, [_P, _I, _c.POINTER(_P)]),
    ("hbh_pool_set_pairing_impl", _I, [_P, _I]),
    ("hbh_pool_verify_sig_shares", _I, [_P, _SZ, _P, _P, _P, _SZ, _P, _P]),
    ("hbh_pool_verify_dec_shares", _I, [_P, _SZ, _P, _P, _P, _P, _SZ, _P, _P]),
    ("hbh_pool_combine_verify_g2", _I, [_P, _SZ, _I, _P, _P, _P, _P, _P, _P, _P]),
    ("hbh_pool_interpolate_g1", _I, [_P, _SZ, _I, _P, _P, _P, _P]),
    ("hbh_pool_bivar_ack_check", _I, [_P, _SZ, _I, _SZ, _P, _P, _P, _P, _P, _P]),
    # host stage (no engine, no GPU)
    ("hbh_host_last_error", _c.c_char_p, []),
    ("hbh_host_threads", _I, [_c.POINTER(_I)]),
    ("hbh_hash_g2", _I, [_SZ, _P, _P, _P, _I]),
    ("hbh_hash_g1_g2", _I, [_SZ, _P, _P, _P, _P, _I]),
    ("hbh_xor_with_hash", _I, [_SZ, _P, _P, _P, _P, _I]),
    ("hbh_signature_parity", _I, [_SZ, _P, _P]),
    ("hbh_g1_compress", _I, [_SZ, _P, _P]),
    ("hbh_g2_compress", _I, [_SZ, _P, _P]),
    ("hbh_host_g1_mul", _I, [_SZ, _P, _P, _P, _I]),
    ("hbh_host_g2_mul", _I, [_SZ, _P, _P, _P, _I]),
    ("hbh_host_g1_add", _I, [_SZ, _P, _P, _P]),
    ("hbh_encrypt", _I, [_SZ, _P, _I, _P, _P, _P, _P, _P, _P, _I]),
    ("hbh_encrypt_uv", _I, [_SZ, _P, _I, _P, _P, _P, _P, _P, _I]),
    ("hbh_encrypt_w", _I, [_SZ, _P, _P, _P, _I]),
    ("hbh_fr_poly_eval", _I, [_SZ, _SZ, _P, _SZ, _P, _P, _I]),
    ("hbh_hash_g1_g2_bp", _I, [_SZ, _P, _P, _P, _P, _I]),
    ("hbh_hash_bp_g1", _I, [_P]),
]
STAGE_PREPARE, STAGE_PAIRING, STAGE_CURVE, STAGE_HASH = 0, 1, 2, 4  # HBH_STAGE_* (3 is not assigned)
IMPL_AUTO, IMPL_PAIR, IMPL_WAVE, IMPL_QUAD, IMPL_OCT, IMPL_WAVE2 = 3, 4, 5, 6, 7, 8   # HBH_IMPL_* (0, 1, 2 = retired THREAD, LANE_COOP, THREAD_SIGNED)
IMPL_WAVEP = 10  # HBH_IMPL_WAVEP (9 is not assigned)
AUTO_WAVEP_MIN, AUTO_WAVEP_MAX = 1025, 1536  # HBH_AUTO_WAVEP_* (profiles/r08: the sizes where WAVEP beats WAVE by more than the spread)
ACK_AUTO, ACK_QUAD, ACK_LANE, ACK_LANE_HORNER = 0, 1, 2, 3  # HBH_ACK_*
DEC_AUTO, DEC_LANE, DEC_SPLIT = 0, 1, 2  # HBH_DEC_*
AUTO_DEC_G1_SPLIT_MAX, AUTO_DEC_G2_SPLIT_MAX = 8192, 8192  # HBH_AUTO_DEC_G*_SPLIT_MAX
HASH_AUTO, HASH_HOST, HASH_DEVICE = 0, 1, 2  # HBH_HASH_*
HASH_ROUNDS = 32  # HBH_HASH_ROUNDS
AUTO_HASH_DEVICE_MIN = 384  # HBH_AUTO_HASH_DEVICE_MIN (profiles/r24: the quad form beats the host stage from here)
HFORM_AUTO, HFORM_LANE, HFORM_QUAD = 0, 1, 2  # HBH_HFORM_*: lanes per message of the device hash
HASH_QUAD_ALL = 2**64 - 1  # HBH_HASH_QUAD_ALL: the value of AUTO_HASH_QUAD_MAX that means every size
AUTO_HASH_QUAD_MAX = HASH_QUAD_ALL  # HBH_AUTO_HASH_QUAD_MAX (0: never; profiles/r24: QUAD wins at every swept size)
GSUM_AUTO, GSUM_CHAIN, GSUM_BUCKET = 0, 1, 2  # HBH_GSUM_*
AUTO_GSUM_G1_BUCKET_MIN, AUTO_GSUM_G2_BUCKET_MIN = 0, 0  # HBH_AUTO_GSUM_G*_BUCKET_MIN (0: never; profiles/r17)
GSCALAR_INT128, GSCALAR_DIGITS = 0, 1  # HBH_GSCALAR_*: how a grouped call reads and draws its scalars
GFORM_INT128, GFORM_X4, GFORM_X2 = 0, 1, 2  # HBH_GFORM_* (hbh_dbg_group_sums_form)
BATCH_GROUP = 256  # HBH_BATCH_GROUP: items per final exponentiation of the batched independent checks
GROUP_TILE = 128  # csrc/group_plan.hpp GROUP_TILE: items per tile of the grouped share checks' sums


class GroupedStats(ctypes.Structure):
    """hbh_grouped_stats"""
    _fields_ = [("groups", ctypes.c_uint32), ("groups_passed", ctypes.c_uint32), ("singles", ctypes.c_uint32),
                ("fallback_items", ctypes.c_uint32)]


_lib = None


class HbhError(RuntimeError):
    pass


def lib():
    """Load libhbbft_hip.so (raises if absent - no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HbhError("libhbbft_hip.so not built (run __graft_entry__.build() or `make -C hbbft_amd`)")
        l = ctypes.CDLL(LIB_PATH)
        for name, res, args in SIGNATURES:
            f = getattr(l, name)
            f.restype = res
            f.argtypes = args
        _lib = l
    return _lib


def check(rc):
    if rc != 0:
        raise HbhError("hbbft_hip error %d: %s" % (rc, lib().hbh_last_error().decode()))


def check_host(rc):
    if rc != 0:
        raise HbhError("hbbft_hip host stage error %d: %s" % (rc, lib().hbh_host_last_error().decode()))


def buf(b):
    """bytes-like -> (ctypes buffer, pointer) kept alive by the caller."""
    if b is None:
        return None, None
    if isinstance(b, (bytes, bytearray, memoryview)):
        cb = (ctypes.c_uint8 * len(b)).from_buffer_copy(bytes(b))
        return cb, ctypes.cast(cb, ctypes.c_void_p)
    raise TypeError(type(b))
