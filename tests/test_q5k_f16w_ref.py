"""tests/q5k_f16w_ref.py checked on the CPU: the numpy restatement of the Q5_K form of k_gemm_f16w dequantizes like the oracle, its A'
stays inside the stated bound, its integer dot is the reference's block dot, the lanes' loads land on B' slot order 3 (the order
Q2_K / Q3_K read), and single mutations of the restatement are told apart from it on the inputs the GPU tests use."""
import numpy as np
import pytest

from crabml_amd import synth
from oracle import oracle as o
from tests import q5k_f16w_ref as Q
from tests import test_hip_f16w_gemm as G

FMT = Q.FMT


def _inputs():
    rng = np.random.default_rng(11)
    return {"random": synth.random_blocks(rng, 64 * 256, synth.Q5_K), "codes": Q.code_blocks(rng), "ints": Q.int_weights(rng, FMT, 8, 2048)}


def test_w_is_the_oracles_dequantize_and_a_is_inside_the_bound():
    for name, raw in _inputs().items():
        n = raw.size // 176 * 256
        ap, w, ea = Q.weight_operands(raw, FMT, range(n // 256), 256)
        ref = o.dequantize(raw, synth.Q5_K).reshape(-1, 256)
        # (the oracle returns f32: d sc q, 11 + 6 + 5 bits, and dmin m are exact there, so that their difference rounds once)
        assert np.array_equal(w.astype(np.float32), ref), (name, np.max(np.abs(w - ref)))
        assert np.all(np.isfinite(ap)) and np.all(np.abs(ap - w) <= ea), (name, np.max(np.abs(ap - w) / ea))


def test_integer_dot_is_the_reference_block_dot():
    """integer blocks against integer rows that quantize to themselves: x . A' in float64 equals the oracle's Q5_K x Q8_K vec_dot (every
    term an integer below 2^24: the f32 block sums of the reference are exact)"""
    rng = np.random.default_rng(5)
    m, k = 4, 1024
    raw = Q.int_weights(rng, FMT, m, k)
    ap, w, _ = Q.weight_operands(raw, FMT, range(m), k)
    assert np.all(ap == np.round(ap)) and np.array_equal(ap, w)
    assert 31 * 3 >= np.abs(ap).max() >= 31 and ap.min() < 0
    with Q.q5k_operands():
        x = G.int_rows(rng, FMT, 2, k)
        bp, _, _, qb = G.row_operands(x, FMT, 2, k)
        assert np.array_equal(bp, x.reshape(2, k).astype(np.float64))
        assert np.array_equal(G.weight_operands(raw, FMT, range(m), k)[0], ap)
    rb = k // 256 * 176
    for r in range(m):
        for i in range(2):
            ref = o.vec_dot(raw[r * rb:(r + 1) * rb], synth.Q5_K, qb[i].reshape(-1), k)
            assert float(ref) == float(bp[i] @ ap[r]), (r, i, ref, bp[i] @ ap[r])
    assert FMT not in G.ROWS and FMT not in G.HT and G.KQ == ("Q4_K", "Q6_K")  # (the substitution ends with the block)


def test_code_blocks_hit_every_code_in_every_sub_block_and_both_qh_states():
    b = Q.code_blocks(np.random.default_rng(3)).reshape(-1, 176)
    sc, mn = Q.scale_codes(b[:, 160:172])
    for j in range(8):
        assert set(sc[:, j]) == set(range(64)) and set(mn[:, j]) == set(range(64)), j
    assert np.array_equal(Q.pack_codes(sc, mn), b[:, 160:172])
    hb = Q.fifth_bits(b[:, 128:160].astype(np.int64)).reshape(-1, 4, 2, 32)
    nib = Q.nibbles(b[:, 0:128]).reshape(-1, 4, 2, 32)
    for p in range(4):
        for hi in range(2):
            assert set(hb[:, p, hi].reshape(-1)) == {0, 1} and set(nib[:, p, hi].reshape(-1)) == set(range(16)), (p, hi)
    assert {0, 0x80} == set(b[:, 173] & 0x80) == set(b[:, 175] & 0x80)  # either sign of d and of dmin


def test_the_lanes_loads_land_on_slot_order_3():
    """the lane's (pair, piece, nibble, qh bit) permutation pushed through order 3's position arithmetic is the identity on all 256
    elements: Q5_K reads the B' that k_rows_to_f16<3>, the row quantizer and k_norm_quant_rows_k write for Q2_K / Q3_K"""
    elem, pos, qh_bit = Q.lane_slots()
    assert sorted(elem) == list(range(256)) and sorted(pos) == list(range(256))
    assert np.array_equal(Q.order3_pos(elem), pos)
    for e, (l, bit) in zip(elem, qh_bit):  # the fifth bit the kernel takes is the element's: bit 2 p + hi of qh[l]
        p, hi = e >> 6, (e >> 5) & 1
        assert (l, bit) == (e & 31, 2 * p + hi), e
    # order3_pos is f16w_pos_q8k(3, ...): the inverse of rows_to_f16_piece<3>'s gather (slot group kb = 4 cc + g, step s, slot e reads
    # element 128 (g >> 1) + 64 (cc & 1) + 16 (g & 1) + 4 s + at[e], at = 0, 2, 1, 3, + 32 for e >= 4)
    for kb in range(8):
        for s in range(4):
            for e in range(8):
                cc, g = kb >> 2, kb & 3
                E = 128 * (g >> 1) + 64 * (cc & 1) + 16 * (g & 1) + 4 * s + (32 if e >= 4 else 0) + ((e >> 1) & 1) + 2 * (e & 1)
                assert Q.order3_pos(E) == kb * 32 + 8 * s + e


@pytest.mark.parametrize("wrong", Q.WRONG)
def test_single_mutations_are_told_apart(wrong):
    """every mutation changes A' on every kind of input the GPU tests use: on the integer blocks the exact tier's integer dot moves (small
    integer rows against the row), on the random and the code blocks A' leaves the bound against W"""
    for name, raw in _inputs().items():
        nsb = raw.size // 176
        ap, w, ea = Q.weight_operands(raw, FMT, range(nsb), 256)
        bad = Q.weight_operands(raw, FMT, range(nsb), 256, wrong)[0]
        assert not np.array_equal(ap, bad), (wrong, name)
        if name == "ints":
            x = np.random.default_rng(1).integers(-8, 9, (4, 256)).astype(np.float64)
            assert not np.array_equal(x @ ap.T, x @ bad.T), wrong
        else:
            assert np.any(np.abs(bad - w) > ea), (wrong, name)
