// A small circuit builder for the WIDE gate  qL a + qR b + qM a b + qH a^5 - qO c + qC + in = 0  that emits the PlonkCircuit `preprocess`
// and `witness_plan` take -- the compiled mirror of zkhip/circuit.py, which carries the full text.  Variables are integers (Var); an
// operand whose coefficient is zero may be kNoVar.  Every row call appends ONE row and returns the variable that names its c:
//     pub()                                   an input row (qO = 1, c = the public input); must precede every other row
//     lin(ka, x, kb, y, kc)                   c = ka x + kb y + kc
//     mul(x, y, k, kc)                        c = k x y + kc
//     pow5(x, kc)                             c = x^5 + kc
//     assert_zero_of(ka, x, kb, y, km, kc)    a non-computing row (qO = 0): ka x + kb y + km x y + kc = 0; its c is tied to nothing
//     assert_bool(x)                          x x - x = 0
//     inv0(x)                                 an ADVICE row (include/zkhip.h): every selector 0, code ZK_ADV_INV0, c = 1 / x, or 0 for x = 0
//     bits_of(x, shift, width)                an advice row, code ZK_ADV_BITS(shift, width): c = bits shift .. shift + width - 1 of x
// An advice row constrains nothing; the gadgets on it add the gate rows that do (rows appended in brackets; zkhip/circuit.py has the text):
//     inverse(x) [2], div(n, d) [3], assert_nonzero(x) [2], is_zero(x) [3], is_equal(x, y) [4], select(bit, x, y) [3],
//     to_bits(x, n) [3n - 1; 1 <= n <= 253; x a computed value], assert_range(x, n) [3n - 1], less_than(x, y, n) [3n + 4; n <= 252]
// priv() is a free variable (no row; its value comes from free[smallest slot of its class]); assert_equal(x, y) joins two copy classes.
// build(): the public rows padded with zero input rows to l = 2^k (1 without any), then the rows in call order; mu the smallest with
// N >= rows and N >= 2 l (mu >= 1); unused rows all-zero; PlonkCircuit::advice is filled only when an advice row was used.  sigma: ONE cycle per class over its slots (column * N + row) in increasing
// order, every other slot a fixed point -- the same array as the Python builder's, so both hosts print one digest.
#pragma once
#include <algorithm>
#include <map>

#include "plonk.hpp"

namespace zkhost {

using Var = long long;
static constexpr Var kNoVar = -1;

struct CircuitLayout {
    size_t mu = 0, N = 0, l = 0, rows = 0;
    std::vector<long long> slot_of, row_of;  // per variable: the smallest slot of its class / the row whose c it names (-1: none)
    size_t slot(Var v) const {
        if (v < 0 || (size_t)v >= slot_of.size() || slot_of[(size_t)v] < 0) throw ZkError(ZK_ERR_INVALID, "circuit layout: the variable has no slot");
        return (size_t)slot_of[(size_t)v];
    }
    size_t row(Var v) const {
        if (v < 0 || (size_t)v >= row_of.size() || row_of[(size_t)v] < 0) throw ZkError(ZK_ERR_INVALID, "circuit layout: the variable names no row");
        return (size_t)row_of[(size_t)v];
    }
    // {private variable, value} pairs -> the 3N `free` elements of plonk_witness
    FrVec free(const std::vector<std::pair<Var, Fr>> &values) const {
        FrVec out(3 * N, Fr::zero());
        for (const auto &kv : values) out[slot(kv.first)] = kv.second;
        return out;
    }
};

class CircuitBuilder {
  public:
    Var pub() {
        if (!rows_.empty()) throw ZkError(ZK_ERR_INVALID, "circuit builder: pub() must precede every other row");
        const Var v = fresh();
        c_row_[(size_t)v] = {true, publics_++};
        return v;
    }
    Var priv() { return fresh(); }
    Var lin(const Fr &ka, Var x, const Fr &kb, Var y, const Fr &kc = Fr::zero()) {
        return row({ka, kb, Fr::zero(), Fr::one(), kc, Fr::zero()}, var(x, !ka.is_zero()), var(y, !kb.is_zero()), true);
    }
    Var mul(Var x, Var y, const Fr &k = Fr::one(), const Fr &kc = Fr::zero()) {
        return row({Fr::zero(), Fr::zero(), k, Fr::one(), kc, Fr::zero()}, var(x, true), var(y, true), true);
    }
    Var pow5(Var x, const Fr &kc = Fr::zero()) { return row({Fr::zero(), Fr::zero(), Fr::zero(), Fr::one(), kc, Fr::one()}, var(x, true), kNoVar, true); }
    void assert_zero_of(const Fr &ka, Var x, const Fr &kb, Var y, const Fr &km, const Fr &kc) {
        row({ka, kb, km, Fr::zero(), kc, Fr::zero()}, var(x, !ka.is_zero() || !km.is_zero()), var(y, !kb.is_zero() || !km.is_zero()), false);
    }
    void assert_bool(Var x) { assert_zero_of(-Fr::one(), x, Fr::zero(), x, Fr::one(), Fr::zero()); }
    // ---- advice rows and the gadgets on them ----
    Var inv0(Var x) { return row(no_sel(), var(x, true), kNoVar, true, ZK_ADV_INV0); }
    Var bits_of(Var x, size_t shift, size_t width) {
        if (width < 1 || width > 64 || shift + width > 255) throw ZkError(ZK_ERR_INVALID, "circuit builder: no advice code for this shift and width");
        return row(no_sel(), var(x, true), kNoVar, true, ZK_ADV_BITS(shift, width));
    }
    Var inverse(Var x) {
        const Var i = inv0(x);
        assert_zero_of(Fr::zero(), x, Fr::zero(), i, Fr::one(), -Fr::one());
        return i;
    }
    Var div(Var n, Var d) { return mul(n, inverse(d)); }
    void assert_nonzero(Var x) { inverse(x); }
    Var is_zero(Var x) {
        const Var z = mul(x, inv0(x), -Fr::one(), Fr::one());
        assert_zero_of(Fr::zero(), x, Fr::zero(), z, Fr::one(), Fr::zero());
        return z;
    }
    Var is_equal(Var x, Var y) { return is_zero(lin(Fr::one(), x, -Fr::one(), y)); }
    Var select(Var bit, Var x, Var y) { return lin(Fr::one(), y, Fr::one(), mul(bit, lin(Fr::one(), x, -Fr::one(), y))); }
    std::vector<Var> to_bits(Var x, size_t n) {
        if (n < 1 || n > 253) throw ZkError(ZK_ERR_INVALID, "circuit builder: to_bits takes 1 <= n <= 253 bits: above that the decomposition would not be unique");
        std::vector<Var> bits;
        for (size_t k = 0; k < n; ++k) bits.push_back(bits_of(x, k, 1));
        for (Var v : bits) assert_bool(v);
        Var acc = bits[0];
        Fr pw = Fr::one();
        for (size_t k = 1; k < n; ++k) {
            pw += pw;
            acc = lin(Fr::one(), acc, pw, bits[k]);
        }
        assert_equal(acc, x);
        return bits;
    }
    void assert_range(Var x, size_t n) { to_bits(x, n); }
    Var less_than(Var x, Var y, size_t n) {
        if (n < 1 || n > 252) throw ZkError(ZK_ERR_INVALID, "circuit builder: less_than takes 1 <= n <= 252 bits");
        Fr pw = Fr::one();
        for (size_t k = 0; k < n; ++k) pw += pw;
        const Var top = to_bits(lin(Fr::one(), x, -Fr::one(), y, pw), n + 1)[n];
        return lin(-Fr::one(), top, Fr::zero(), kNoVar, Fr::one());
    }
    void assert_equal(Var x, Var y) {
        const size_t rx = find((size_t)var(x, true)), ry = find((size_t)var(y, true));
        if (rx != ry) parent_[std::max(rx, ry)] = std::min(rx, ry);
    }

    PlonkCircuit build(CircuitLayout &layout) {
        size_t l = 1;
        while (l < publics_) l *= 2;
        const size_t rows = l + rows_.size();
        size_t mu = 1;
        while ((size_t(1) << mu) < rows || (size_t(1) << mu) < 2 * l) ++mu;
        const size_t N = size_t(1) << mu;
        PlonkCircuit c;
        c.gate = GateKind::wide, c.mu = mu, c.l = l;
        c.sel.assign(6, FrVec(N, Fr::zero()));
        for (size_t x = 0; x < l; ++x) c.sel[3][x] = Fr::one();
        std::map<size_t, std::vector<size_t>> slots;  // class -> its slots
        layout = CircuitLayout{mu, N, l, rows, std::vector<long long>(parent_.size(), -1), std::vector<long long>(parent_.size(), -1)};
        for (size_t v = 0; v < parent_.size(); ++v)
            if (c_row_[v].second != kNone) {
                const size_t x = c_row_[v].first ? c_row_[v].second : l + c_row_[v].second;
                layout.row_of[v] = (long long)x;
                slots[find(v)].push_back(2 * N + x);
            }
        for (size_t i = 0; i < rows_.size(); ++i) {
            const size_t x = l + i;
            for (size_t k = 0; k < 6; ++k) c.sel[k][x] = rows_[i].sel[k];
            if (rows_[i].advice) {
                if (c.advice.empty()) c.advice.assign(N, 0);
                c.advice[x] = rows_[i].advice;
            }
            if (rows_[i].a != kNoVar) slots[find((size_t)rows_[i].a)].push_back(x);
            if (rows_[i].b != kNoVar) slots[find((size_t)rows_[i].b)].push_back(N + x);
        }
        c.sigma.resize(3 * N);
        for (size_t s = 0; s < 3 * N; ++s) c.sigma[s] = s;
        for (auto &kv : slots) {
            std::vector<size_t> &ss = kv.second;
            std::sort(ss.begin(), ss.end());
            for (size_t i = 0; i < ss.size(); ++i) c.sigma[ss[i]] = ss[(i + 1) % ss.size()];
        }
        for (size_t v = 0; v < parent_.size(); ++v) {
            auto it = slots.find(find(v));
            if (it != slots.end()) layout.slot_of[v] = (long long)it->second[0];
        }
        return c;
    }

  private:
    static constexpr size_t kNone = ~size_t(0);
    struct Row {
        std::array<Fr, 6> sel;  // qL, qR, qM, qO, qC, qH
        Var a, b;
        uint32_t advice;
    };
    static std::array<Fr, 6> no_sel() { return {Fr::zero(), Fr::zero(), Fr::zero(), Fr::zero(), Fr::zero(), Fr::zero()}; }
    Var fresh() {
        parent_.push_back(parent_.size());
        c_row_.push_back({false, kNone});
        return (Var)parent_.size() - 1;
    }
    size_t find(size_t v) {
        while (parent_[v] != v) v = parent_[v] = parent_[parent_[v]];
        return v;
    }
    Var var(Var v, bool needed) const {
        if (v == kNoVar) {
            if (needed) throw ZkError(ZK_ERR_INVALID, "circuit builder: an operand with a non-zero coefficient is needed");
            return v;
        }
        if (v < 0 || (size_t)v >= parent_.size()) throw ZkError(ZK_ERR_INVALID, "circuit builder: not a variable of this builder");
        return v;
    }
    Var row(const std::array<Fr, 6> &sel, Var a, Var b, bool computing, uint32_t advice = 0) {
        Var c = kNoVar;
        if (computing) {
            c = fresh();
            c_row_[(size_t)c] = {false, rows_.size()};
        }
        rows_.push_back({sel, a, b, advice});
        return c;
    }
    size_t publics_ = 0;
    std::vector<Row> rows_;
    std::vector<size_t> parent_;
    std::vector<std::pair<bool, size_t>> c_row_;  // per variable: (an input row?, its index) or kNone
};

// SHA-256 of a built circuit: mu and l (one u64 each), the six selectors, sigma (u64) and, only when it has them, the advice codes (u32),
// little-endian (zkhip.circuit.circuit_digest)
inline std::string built_circuit_digest(const PlonkCircuit &c) {
    Sha256 h;
    const uint64_t head[2] = {c.mu, c.l};
    h.update(head, 16);
    for (const FrVec &q : c.sel) h.update(q.data(), 32 * q.size());
    h.update(c.sigma.data(), 8 * c.sigma.size());
    if (!c.advice.empty()) h.update(c.advice.data(), 4 * c.advice.size());
    return h.hex();
}

}  // namespace zkhost
