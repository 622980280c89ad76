"""
The integer model of the G2 validation (g2check_model.py) against itself and against the Python host's rule (zkhip.serialize): the psi
constants, Scott's rule psi(P) == [x]P against the definition [r]P = O on every kind of point, the encoding of the generator, and
serialize.g2_decompress_check_host against the model on the whole case list.  No device.
"""
import numpy as np

import g2check_model as gm


def test_psi_of_the_generator_is_q_times_the_generator():
    assert gm.on_curve(gm.G2) and gm.in_g2(gm.G2)
    assert gm.psi(gm.G2) == gm.mul(gm.G2, gm.Q % gm.R)
    assert gm.Q % gm.R == gm.R - gm.X_ABS  # q = x (mod r), x negative


def test_the_psi_rule_agrees_with_the_definition_on_every_kind_of_point():
    kinds = set()
    for name, P in gm.points(1):
        assert gm.on_curve(P), name
        assert gm.psi_rule(P) == gm.in_g2(P), name
        assert gm.in_g2(P) == name.startswith(("member", "infinity")), name
        kinds.add(name)
    assert {"member", "twist", "cofactor", "cofactor+kG", "order13", "order23", "infinity"} <= kinds


def test_small_order_points_have_their_order():
    pts = dict((n, P) for n, P in gm.points(1) if n in ("order13", "order23"))
    assert gm.mul(pts["order13"], 13) is None and pts["order13"] is not None
    assert gm.mul(pts["order23"], 23) is None and pts["order23"] is not None


def test_the_encoding_of_the_generator_and_the_round_trip():
    from zkhip import pairing as pr

    assert pr.G2_GEN == gm.G2
    e = gm.compress(gm.G2)
    assert len(e) == 96 and e[0] == 0x93  # compressed, sign clear (y.c1 <= (q - 1) / 2), the top byte of x.c1
    assert gm.G2[1][1] <= gm.HALF
    assert int.from_bytes(bytes([e[0] & 0x1F]) + e[1:48], "big") == gm.G2[0][1] and int.from_bytes(e[48:], "big") == gm.G2[0][0]
    for name, enc in gm.cases(1):
        st, P = gm.decompress_check(enc)
        if st in (gm.OK, gm.NOT_IN_G2):
            assert gm.compress(P) == enc, name


def test_the_two_roots_of_one_x_decode_to_p_and_minus_p():
    for name, P in gm.points(1):
        if P is None:
            continue
        e = bytearray(gm.compress(P))
        e[0] ^= 0x20
        assert gm.decompress_check(bytes(e))[1] == gm.neg(P), name
        assert gm.y_is_larger(P[1]) != gm.y_is_larger(gm.neg(P)[1])
    # the sign rule when y.c1 = 0: c0 decides
    assert gm.y_is_larger((gm.HALF + 1, 0)) and not gm.y_is_larger((gm.HALF, 0)) and not gm.y_is_larger((gm.Q - 1, 1)) and gm.y_is_larger((0, gm.HALF + 1))


def test_the_python_host_rule_equals_the_model_on_the_whole_case_list():
    from zkhip import serialize as ser

    assert ser.PSI_CX == gm.C_X and ser.PSI_CY == gm.C_Y
    encs = [e for _, e in gm.cases(1)]
    want_pts, want_st = gm.expected(encs)
    assert set(want_st.tolist()) == {0, 1, 2, 3}
    pts, st = ser.g2_decompress_check_host(b"".join(encs))
    bad = [(n, int(a), int(b)) for (n, _), a, b in zip(gm.cases(1), st, want_st) if a != b]
    assert not bad, bad
    assert (pts == want_pts).all()
    for (name, e), s in zip(gm.cases(1), want_st):
        if s in (gm.OK, gm.NOT_IN_G2):
            P = ser.g2_deserialize_compressed(e)
            assert P == gm.decompress_check(e)[1] and ser.g2_serialize_compressed(P) == e, name
            assert ser.g2_in_subgroup(P) == (s == gm.OK), name
            assert (ser.g2_point_words(P) == gm.words(P)).all()
    assert ser._g2_y_is_larger((gm.HALF + 1, 0)) and not ser._g2_y_is_larger((gm.HALF, 0))
