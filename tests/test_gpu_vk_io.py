"""
Verifying-key bytes end to end on the device (zkhip.vk_io): prove at mu = 4 for the basic and the wide gate, with and without the lookup
sample; the vk read back from its bytes verifies the proof through verify, verify_agg and verify_files; the device and the host path give
one dict and the same errors; a key plus a point of small order is refused by name; a flipped bit in any commitment or key gives a
refusal or a False verdict, never True.
"""
import numpy as np
import pytest

import g2check_model as gm
import zerocheck_model as zm

pytestmark = pytest.mark.gpu

MU = 4
KINDS = [(None, False), (None, True), ("wide", False), ("wide", True)]
_PROVED = {}


def _proved(ctx, kind, lookup):
    """(vk, public inputs, record, vk bytes, proof bytes, public bytes), proved once per kind"""
    if (kind, lookup) not in _PROVED:
        from zkhip import dist_primitive as dp
        from zkhip import pairing as pr
        from zkhip import plonk, vk_io

        if lookup:
            c = plonk.sample_circuit_lookup(MU, 31, gate=kind)
        else:
            c = (plonk.sample_circuit_wide if kind else plonk.sample_circuit)(MU, 31)
        pcs = dp.PolynomialCommitmentCub.new(ctx, c["s"]).mature()
        pk, vk = plonk.preprocess(ctx, pcs, c, pr.powers_of_g2(zm.ints(c["s"])))
        proof = plonk.prove(ctx, pk, c["a"], c["b"], c["c"], c["public_inputs"], **({"idx": c["idx"]} if lookup else {}))
        _PROVED[(kind, lookup)] = (vk, c["public_inputs"], proof, plonk.vk_to_bytes(vk), plonk.proof_to_bytes(proof), vk_io.public_to_bytes(c["public_inputs"]))
    return _PROVED[(kind, lookup)]


def _message(fn):
    with pytest.raises(ValueError) as e:
        fn()
    return str(e.value)


@pytest.mark.parametrize("kind,lookup", KINDS)
def test_the_vk_of_the_bytes_verifies_what_the_original_verifies(ctx, kind, lookup):
    from zkhip import plonk, vk_io

    vk, pi, proof, vkb, pfb, pib = _proved(ctx, kind, lookup)
    assert vk["g2"].shape == (MU + 2, 24) and len(vkb) == vk_io.vk_size(kind, lookup, MU)
    assert plonk.check_vk(ctx, vk) == []
    back = plonk.vk_from_bytes(ctx, vkb)
    host = plonk.vk_from_bytes(ctx, vkb, host=True)
    for d in (back, host):
        assert set(d) == set(vk)
        assert all((d[k] == vk[k]).all() for k in ("commitments", "g2")) and all(d.get(k) == vk.get(k) for k in ("mu", "l", "gate", "lookup"))
    assert plonk.vk_to_bytes(back) == vkb
    assert plonk.verify(ctx, vk, pi, proof) is True
    assert plonk.verify(ctx, back, pi, proof) is True and plonk.verify_agg(ctx, back, pi, proof) is True
    assert plonk.verify_files(ctx, vkb, pfb, pib) is True and plonk.verify_files(ctx, vkb, pfb, pib, aggregate=True) is True
    assert plonk.verify_files(ctx, vkb, pfb, pib, host=True) is True
    # other public inputs: a False verdict; public bytes of another length or not canonical: refused
    other = bytearray(pib)
    other[0] ^= 1
    assert plonk.verify_files(ctx, vkb, pfb, bytes(other)) is False
    assert "public inputs" in _message(lambda: plonk.verify_files(ctx, vkb, pfb, pib + bytes(32)))
    assert "public input 0" in _message(lambda: plonk.verify_files(ctx, vkb, pfb, b"\xff" * 32 + pib[32:]))


@pytest.mark.parametrize("kind,lookup", KINDS)
def test_a_key_plus_a_small_order_point_is_refused_by_name_on_both_paths(ctx, kind, lookup):
    from zkhip import plonk, vk_io

    vk, pi, proof, vkb, pfb, pib = _proved(ctx, kind, lookup)
    k = vk_io.commitment_count(kind, lookup)
    small = dict(gm.points(1))
    for j, name in ((0, "order13"), (1 + (1 if lookup else 0), "order23"), (MU + 1, "order13")):
        at = 26 + 48 * k + 96 * j
        P = gm.add(gm.decompress_check(bytes(vkb[at:at + 96]))[1], small[name])
        assert gm.on_curve(P) and not gm.in_g2(P)
        bad = vkb[:at] + gm.compress(P) + vkb[at + 96:]
        want = f"G2 key {j}: not in the subgroup"
        assert _message(lambda: plonk.vk_from_bytes(ctx, bad)) == want
        assert _message(lambda: plonk.vk_from_bytes(ctx, bad, host=True)) == want
        assert _message(lambda: plonk.verify_files(ctx, bad, pfb, pib)) == want
        rec = dict(vk, g2=vk["g2"].copy())
        rec["g2"][j] = gm.words(P)
        assert plonk.check_vk(ctx, rec) == [want]
        inf = vkb[:at] + gm.compress(None) + vkb[at + 96:]
        assert _message(lambda: plonk.vk_from_bytes(ctx, inf)) == _message(lambda: plonk.vk_from_bytes(None, inf, host=True)) == f"G2 key {j}: the point at infinity"
        rec["g2"][j] = 0
        assert plonk.check_vk(ctx, rec) == [f"G2 key {j}: the point at infinity"]


@pytest.mark.parametrize("kind,lookup", KINDS)
def test_a_flipped_bit_in_any_commitment_or_key_never_verifies(ctx, kind, lookup):
    from zkhip import plonk, vk_io

    vk, pi, proof, vkb, pfb, pib = _proved(ctx, kind, lookup)
    k = vk_io.commitment_count(kind, lookup)
    rng = np.random.default_rng(5 + k)
    spans = [(26 + 48 * j, 48) for j in range(k)] + [(26 + 48 * k + 96 * j, 96) for j in range(MU + 2)]
    for pos, size in spans:
        at = pos + int(rng.integers(size))
        bad = bytearray(vkb)
        bad[at] ^= 1 << int(rng.integers(8))
        try:
            verdict = plonk.verify_files(ctx, bytes(bad), pfb, pib)
        except ValueError as e:
            dev = str(e)
            assert _message(lambda: plonk.vk_from_bytes(None, bytes(bad), host=True)) == dev, at
            continue
        assert verdict is False, at
    assert plonk.verify_files(ctx, vkb, pfb, pib) is True
