"""
The inputs of the transfer circuit (zkhip.poseidon.merkle_transfer_circuit) for test_advice.py and test_gpu_transfer.py: a tree of balances
by the host rules, one good transfer and the four that must be refused, and what the model of the rules (advice_model.py) reports on each.
"""
import numpy as np

import advice_model as am
import witness_model as wm

# name -> (a bad gate row?, a bad copy?) on the generated witness
EXPECTED = {"good": (False, False), "zero": (True, False), "over": (False, True), "overflow": (False, True), "sibling": (False, True)}


def case(depth: int, bits: int) -> dict:
    """leaf 0 pays leaf 1.  The balances leave room for one transfer that overflows the receiver alone"""
    from zkhip import poseidon as ps

    circuit, layout, v = ps.merkle_transfer_circuit(depth, bits)
    top = 1 << bits
    balances = ([top - 56, top - 6, 100, 30] + [7] * (1 << depth))[:1 << depth]
    return {"depth": depth, "bits": bits, "circuit": circuit, "layout": layout, "vars": v, "balances": balances,
            "amounts": {"good": 5, "zero": 0, "over": balances[0] + 1, "overflow": 10, "sibling": 5}}


def inputs(case: dict, name: str):
    """-> (public inputs [2, 4], free [3N, 4]) of the named transfer; the roots are those of the honest tree walk with that amount"""
    from zkhip import poseidon as ps
    from zkhip.field import R_MOD, fr_mont

    n, amount, bal = 1 << case["depth"], case["amounts"][name], case["balances"]
    tree = ps.merkle_host(bal)
    old_root, sides = tree[-1], []
    for k, x in ((0, (bal[0] - amount) % R_MOD), (1, (bal[1] + amount) % R_MOD)):
        sibs, bits = ps.merkle_path(tree, n, k)
        sides.append((tree[k], list(sibs), list(bits)))
        tree = ps.update_host(tree, n, [(k, x)])
    if name == "sibling":
        sides[0][1][0] = (sides[0][1][0] + 1) % R_MOD
    pi = np.stack([fr_mont(old_root), fr_mont(tree[-1])])
    return pi, ps.merkle_transfer_inputs(case["layout"], case["vars"], amount, *sides)


def model_report(case: dict, name: str) -> dict:
    pi, free = inputs(case, name)
    p = case.setdefault("plan", am.plan(case["circuit"]))
    a, b, c = am.generate(case["circuit"], p, pi, wm.ints(free))
    return am.check(case["circuit"], p, a, b, c, pi)


def message(rep: dict, N: int) -> str:
    """what zk_plonk_witness says of a witness with this report (include/zkhip.h)"""
    parts = []
    if rep["bad_rows"]:
        parts.append(f"{rep['bad_rows']} of {N} rows do not satisfy the gate; the first is row {rep['first_bad_row']}")
    if rep["bad_copies"]:
        parts.append(f"{rep['bad_copies']} of {3 * N} slots differ from the value of their class; the first is slot {rep['first_bad_copy']}")
    return "zk_plonk_witness: " + "; ".join(parts)
