"""
CPU checks of the device pairing's data and formulas (csrc/fq12.cuh, csrc/pairing_consts.cuh, csrc/zk_pairing.hip):
  * tools/gen_pairing_consts.py reproduces the committed csrc/pairing_consts.cuh;
  * the ark-layout converter of zkhip.pairing is a ring homomorphism from a straight Python model of ark's
    Fq2/Fq6/Fq12 tower to zkhip.pairing's Fq[w]/(w^12 - 2 w^6 + 2), and every generated Frobenius constant is right;
  * the device algorithm, transcribed formula by formula into Python below (projective M-twist Miller loop with sparse
    line multiplication, easy part, Hayashida-Hayasaka-Teruya hard part with Granger-Scott cyclotomic squaring), equals
    zkhip.pairing.pairing ** ZK_PAIRING_EXP_MULTIPLE.
"""
import os
import random
import re
import sys

from zkhip import pairing as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "scalable-collaborative-zksnark_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_pairing_consts as gp  # noqa: E402

Q = pr.Q


# ---- ark's tower, straight -----------------------------------------------------------------------------------------------
def f2add(a, b):
    return ((a[0] + b[0]) % Q, (a[1] + b[1]) % Q)


def f2sub(a, b):
    return ((a[0] - b[0]) % Q, (a[1] - b[1]) % Q)


def f2mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % Q, (a[0] * b[1] + a[1] * b[0]) % Q)


def f2xi(a):  # a (1 + u)
    return ((a[0] - a[1]) % Q, (a[0] + a[1]) % Q)


def f2conj(a):
    return (a[0], (-a[1]) % Q)


def f2inv(a):
    n = pow(a[0] * a[0] + a[1] * a[1], -1, Q)
    return (a[0] * n % Q, (-a[1]) * n % Q)


Z2, O2 = (0, 0), (1, 0)


def f6add(a, b):
    return tuple(f2add(x, y) for x, y in zip(a, b))


def f6sub(a, b):
    return tuple(f2sub(x, y) for x, y in zip(a, b))


def f6mul(a, b):
    t = [Z2] * 5
    for i in range(3):
        for j in range(3):
            t[i + j] = f2add(t[i + j], f2mul(a[i], b[j]))
    return (f2add(t[0], f2xi(t[3])), f2add(t[1], f2xi(t[4])), t[2])


def f6v(a):  # a v
    return (f2xi(a[2]), a[0], a[1])


def f6inv(a):
    c0, c1, c2 = a
    t0 = f2sub(f2mul(c0, c0), f2xi(f2mul(c1, c2)))
    t1 = f2sub(f2xi(f2mul(c2, c2)), f2mul(c0, c1))
    t2 = f2sub(f2mul(c1, c1), f2mul(c0, c2))
    n = f2add(f2mul(c0, t0), f2xi(f2add(f2mul(c2, t1), f2mul(c1, t2))))
    ni = f2inv(n)
    return (f2mul(t0, ni), f2mul(t1, ni), f2mul(t2, ni))


def f12mul(a, b):
    v0, v1 = f6mul(a[0], b[0]), f6mul(a[1], b[1])
    return (f6add(v0, f6v(v1)), f6add(f6mul(a[0], b[1]), f6mul(a[1], b[0])))


def f12conj(a):
    return (a[0], f6sub((Z2, Z2, Z2), a[1]))


def f12inv(a):
    t = f6inv(f6sub(f6mul(a[0], a[0]), f6v(f6mul(a[1], a[1]))))
    return (f6mul(a[0], t), f6sub((Z2, Z2, Z2), f6mul(a[1], t)))


ONE12 = ((O2, Z2, Z2), (Z2, Z2, Z2))


def frob(a, k):
    """b_e w^e -> conj^k(b_e) gamma_{k,e} w^e (the device's Frobenius, the generator's constants)"""
    out = [[None] * 3 for _ in range(2)]
    for i in range(2):
        for j in range(3):
            e = i + 2 * j
            b = a[i][j] if k % 2 == 0 else f2conj(a[i][j])
            out[i][j] = f2mul(b, gp.gamma(k, e)) if e else b
    return (tuple(out[0]), tuple(out[1]))


def to_words(a):
    """model element -> ark's 72 u64"""
    out = []
    for i in range(2):
        for j in range(3):
            for x in a[i][j]:
                m = x * (1 << 384) % Q
                out.extend((m >> (64 * k)) & ((1 << 64) - 1) for k in range(6))
    return out


def to_fq12(a):
    return pr.fq12_from_ark(to_words(a))


def rand12(rng):
    return tuple(tuple((rng.randrange(Q), rng.randrange(Q)) for _ in range(3)) for _ in range(2))


# ---- 1. generated constants -----------------------------------------------------------------------------------------------
def test_generator_reproduces_the_committed_header():
    with open(os.path.join(CSRC, "pairing_consts.cuh")) as f:
        committed = f.read()
    assert gp.render() == committed, "run: python tools/gen_pairing_consts.py > scalable-collaborative-zksnark_amd/csrc/pairing_consts.cuh"


def test_generated_limbs_are_the_internal_montgomery_form():
    src = gp.render()
    m = re.search(r"B3_C0\[13\] = \{([^}]*)\}", src)
    limbs = [int(x.strip().rstrip("u"), 16) for x in m.group(1).split(",")]
    assert sum(v << (30 * i) for i, v in enumerate(limbs)) == 12 * (1 << 390) % Q
    assert gp.EXP_MULTIPLE % pr.R_MOD and pr.R_MOD % gp.EXP_MULTIPLE


# ---- 2. the converter is a ring homomorphism; the Frobenius constants ---------------------------------------------------------
def test_ark_layout_converter_is_a_ring_homomorphism():
    rng = random.Random(20261016)
    for _ in range(6):
        a, b = rand12(rng), rand12(rng)
        assert to_fq12(f12mul(a, b)) == to_fq12(a) * to_fq12(b)
        assert to_fq12(tuple(f6add(x, y) for x, y in zip(a, b))) == to_fq12(a) + to_fq12(b)
        assert pr.fq12_to_ark(to_fq12(a)) == to_words(a)
    assert to_fq12(ONE12) == pr.Fq12.one()
    # the generators of the tower land where the issue's map says: v = w^2, w = w
    assert to_fq12(((Z2, O2, Z2), (Z2, Z2, Z2))) == pr.W * pr.W
    assert to_fq12(((Z2, Z2, Z2), (O2, Z2, Z2))) == pr.W


def test_frobenius_constants():
    rng = random.Random(7)
    a = rand12(rng)
    fa = to_fq12(a)
    for k in (1, 2, 3):
        assert to_fq12(frob(a, k)) == fa ** (Q**k), k


# ---- 3. the device algorithm, formula by formula --------------------------------------------------------------------------------
B3 = (12, 12)  # 3 b'


def mul_by_014(f, c0, c1, c4):
    """f * (c0 + c1 v + c4 v w): the sparse line product of fq12.cuh"""
    a, b = f
    aa = (f2mul(a[0], c0), f2add(f2mul(a[0], c1), f2mul(a[1], c0)), f2add(f2mul(a[1], c1), f2mul(a[2], c0)))
    aa = (f2add(aa[0], f2xi(f2mul(a[2], c1))), aa[1], aa[2])
    bb = (f2xi(f2mul(b[2], c4)), f2mul(b[0], c4), f2mul(b[1], c4))
    s = f6add(a, b)
    o = f2add(c1, c4)
    t = (f2mul(s[0], c0), f2add(f2mul(s[0], o), f2mul(s[1], c0)), f2add(f2mul(s[1], o), f2mul(s[2], c0)))
    t = (f2add(t[0], f2xi(f2mul(s[2], o))), t[1], t[2])
    return (f6add(aa, f6v(bb)), f6sub(f6sub(t, aa), bb))


def dbl_step(T, xp, yp):
    X, Y, Z = T
    a = f2mul(X, Y)  # XY (the device keeps 2x the a of arkworks' formula: no halving)
    b = f2mul(Y, Y)
    c = f2mul(Z, Z)
    e = f2mul(B3, c)  # 3 b' Z^2
    f = f2add(f2add(e, e), e)
    g = f2add(b, f)  # 2 x ((Y^2 + 9 b' Z^2) / 2)
    h = f2sub(f2mul(f2add(Y, Z), f2add(Y, Z)), f2add(b, c))  # 2 Y Z
    i = f2sub(e, b)
    j = f2mul(X, X)
    # (X, Y, Z) scaled by 2: X' = 2 XY/2 (b - f) ... every coordinate x4 (projective: same point)
    X3 = f2mul(f2add(a, a), f2sub(b, f))  # 4 * (XY/2)(b - f)
    Y3 = f2sub(f2mul(g, g), f2mul((12, 0), f2mul(e, e)))  # 4 * ((g/2)^2 - 3 e^2)
    Z3 = f2mul((4, 0), f2mul(b, h))
    line = (i, f2mul(f2add(f2add(j, j), j), (xp, 0)), f2mul(f2sub(Z2, h), (yp, 0)))
    return (X3, Y3, Z3), line


def add_step(T, Qa, xp, yp):
    X, Y, Z = T
    qx, qy = Qa
    theta = f2sub(Y, f2mul(qy, Z))
    lam = f2sub(X, f2mul(qx, Z))
    c = f2mul(theta, theta)
    d = f2mul(lam, lam)
    e = f2mul(lam, d)
    f = f2mul(Z, c)
    g = f2mul(X, d)
    h = f2sub(f2add(e, f), f2add(g, g))
    X3 = f2mul(lam, h)
    Y3 = f2sub(f2mul(theta, f2sub(g, h)), f2mul(e, Y))
    Z3 = f2mul(Z, e)
    j = f2sub(f2mul(theta, qx), f2mul(lam, qy))
    line = (j, f2mul(f2sub(Z2, theta), (xp, 0)), f2mul(lam, (yp, 0)))
    return (X3, Y3, Z3), line


def miller(Qa, P):
    xp, yp = P
    T = (Qa[0], Qa[1], O2)
    f = ONE12
    for bit in bin(gp.X_ABS)[3:]:
        f = f12mul(f, f)
        T, l = dbl_step(T, xp, yp)
        f = mul_by_014(f, *l)
        if bit == "1":
            T, l = add_step(T, Qa, xp, yp)
            f = mul_by_014(f, *l)
    return f


def cyc_sqr(f):
    """Granger-Scott squaring in the cyclotomic subgroup (fq12.cuh's f12_cyc_sqr)"""
    (r0, r4, r3), (r2, r1, r5) = f

    def fq4_sqr(a, b):  # (a + b y)^2, y^2 = xi
        t = f2mul(a, b)
        t0 = f2sub(f2sub(f2mul(f2add(a, b), f2add(f2xi(b), a)), t), f2xi(t))
        return t0, f2add(t, t)

    t0, t1 = fq4_sqr(r0, r1)
    t2, t3 = fq4_sqr(r2, r3)
    t4, t5 = fq4_sqr(r4, r5)
    three = lambda t, z, sgn: f2add(f2add(t, t), f2add(t, f2add(z, z) if sgn > 0 else f2sub(Z2, f2add(z, z))))
    z0 = three(t0, r0, -1)
    z1 = three(t1, r1, +1)
    z2 = three(f2xi(t5), r2, +1)
    z3 = three(t4, r3, -1)
    z4 = three(t2, r4, -1)
    z5 = three(t3, r5, +1)
    return ((z0, z4, z3), (z2, z1, z5))


def exp_by_x(f):
    """f^x, x < 0: f^|x| by cyclotomic squarings, then the conjugate"""
    r = f
    for bit in bin(gp.X_ABS)[3:]:
        r = cyc_sqr(r)
        if bit == "1":
            r = f12mul(r, f)
    return f12conj(r)


def final_exp(f):
    r = f12mul(f12conj(f), f12inv(f))  # f^(q^6 - 1)
    r = f12mul(frob(r, 2), r)  # ^(q^2 + 1)
    y0 = f12conj(cyc_sqr(r))
    y5 = exp_by_x(r)
    y1 = cyc_sqr(y5)
    y3 = f12mul(y0, y5)
    y0 = exp_by_x(y3)
    y2 = exp_by_x(y0)
    y4 = f12mul(exp_by_x(y2), y1)
    y1 = f12mul(f12mul(exp_by_x(y4), f12conj(y3)), r)
    y0 = frob(f12mul(y0, r), 3)
    y4 = frob(f12mul(y4, f12conj(r)), 1)
    y5 = frob(f12mul(y5, y2), 2)
    return f12mul(f12mul(f12mul(y5, y0), y4), y1)


def test_cyclotomic_squaring_is_squaring_in_the_cyclotomic_subgroup():
    rng = random.Random(3)
    a = rand12(rng)
    r = f12mul(f12conj(a), f12inv(a))
    r = f12mul(frob(r, 2), r)
    assert to_fq12(cyc_sqr(r)) == to_fq12(f12mul(r, r))


def test_device_algorithm_equals_the_host_pairing_to_the_fixed_power():
    a, b = 0x1234567, 0x89ABCDEF0123
    P = pr.g1_mul(pr.G1_GEN, a)
    Qp = pr.g2_mul(pr.G2_GEN, b)
    dev = to_fq12(final_exp(miller(Qp, P)))
    assert dev == pr.pairing(Qp, P) ** (gp.EXP_MULTIPLE % pr.R_MOD)
    assert not (dev == pr.Fq12.one())


# ---- 4. the compiled host's verifier (host/examples/pcs_verify.cpp) refuses to run without a GPU -------------------------------
def test_pcs_verify_builds_and_refuses_without_a_gpu():
    import subprocess

    host = os.path.join(ROOT, "scalable-collaborative-zksnark_amd", "host")
    subprocess.check_call(["make", "-C", host, "-s", "bin/pcs_verify"])
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([os.path.join(host, "bin", "pcs_verify")], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "no CPU fallback" in r.stderr, (r.returncode, r.stdout, r.stderr)


# ---- 5. ZK_PAIRING_EXP_MULTIPLE has one value everywhere it is written ------------------------------------------------------------
def test_exp_multiple_agrees_between_generator_header_and_rust():
    hdr = open(os.path.join(ROOT, "include", "zkhip.h")).read()
    rs = open(os.path.join(ROOT, "rust", "zkhip_sys.rs")).read()
    consts = open(os.path.join(CSRC, "pairing_consts.cuh")).read()
    assert int(re.search(r"#define ZK_PAIRING_EXP_MULTIPLE (\d+)", hdr).group(1)) == gp.EXP_MULTIPLE
    assert int(re.search(r"#define ZK_PAIRING_EXP_MULTIPLE (\d+)", consts).group(1)) == gp.EXP_MULTIPLE
    assert int(re.search(r"pub const ZK_PAIRING_EXP_MULTIPLE: i32 = (\d+);", rs).group(1)) == gp.EXP_MULTIPLE
