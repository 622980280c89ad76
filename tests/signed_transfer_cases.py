"""
One signed transfer on a 4-leaf tree for the CPU and the GPU tests of zkhip.jubjub.merkle_signed_transfer_circuit(depth = 2, bits = 8): leaves
hash2(hash2(PK.x, PK.y), balance), everything in the model's integers (jubjub_model.py, poseidon_model.py).  The GPU test builds the same
trees with Poseidon.merkle / update and compares.
"""
import jubjub_model as jm
import poseidon_model as pm

DEPTH, BITS, N = 2, 8, 4
SKS = [11, 22, 33, 44]
BALANCES = [100, 7, 50, 0]
SENDER, RECEIVER, AMOUNT = 2, 1, 30
_cache = {}


def key_hash(PK):
    return pm.hash2(PK[0], PK[1])


def leaf(PK, balance):
    return pm.hash2(key_hash(PK), balance)


def base():
    if "base" not in _cache:
        pks = [jm.keygen(sk) for sk in SKS]
        _cache["base"] = pks, pm.merkle([leaf(P, bal) for P, bal in zip(pks, BALANCES)])
    return _cache["base"]


def message(amount):
    pks, tree = base()
    return pm.hash2(pm.hash2(key_hash(pks[RECEIVER]), amount), tree[-1])


def case(name):
    """-> dict(pi = [old root, new root], amount, pk, receiver_key, sig, sender, receiver, trees): "good"; "receiver_signed": the signature is
    the RECEIVER's key's; "other_amount": the signature is on AMOUNT, the transfer (and its new root) moves AMOUNT + 1"""
    if name in _cache:
        return _cache[name]
    pks, tree0 = base()
    amount = AMOUNT + 1 if name == "other_amount" else AMOUNT
    sig = jm.sign(SKS[RECEIVER] if name == "receiver_signed" else SKS[SENDER], message(AMOUNT))
    leaves = list(tree0[:N])
    leaves[SENDER] = leaf(pks[SENDER], BALANCES[SENDER] - amount)
    tree1 = pm.merkle(leaves)
    leaves[RECEIVER] = leaf(pks[RECEIVER], BALANCES[RECEIVER] + amount)
    tree2 = pm.merkle(leaves)
    s_sib, s_bits = pm.path_of(tree0, N, SENDER)
    r_sib, r_bits = pm.path_of(tree1, N, RECEIVER)
    _cache[name] = dict(pi=[tree0[-1], tree2[-1]], amount=amount, pk=pks[SENDER], receiver_key=key_hash(pks[RECEIVER]), sig=sig,
                        sender=(BALANCES[SENDER], s_sib, s_bits), receiver=(BALANCES[RECEIVER], r_sib, r_bits), trees=(tree0, tree1, tree2))
    return _cache[name]


def free_of(layout, v, c):
    from zkhip import jubjub as jj

    return jj.merkle_signed_transfer_inputs(layout, v, c["amount"], c["pk"], c["receiver_key"], c["sig"], c["sender"], c["receiver"])
