// The sumcheck verifier's round chain -- the compiled counterpart of zkhip.verify.round_poly_at / round_chain, and the ONE copy the
// verifiers of zerocheck.hpp, wiring.hpp, lookup.hpp, batch_open.hpp and plonk.hpp call:
//     p_0(0) + p_0(1) == claimed,   p_i(0) + p_i(1) == p_{i-1}(r_{i-1}),   last = p_{n-1}(r_{n-1})
// with every round polynomial given by its values on the nodes 0 .. K - 1 (K = degree + 1; K = 3 is dsumcheck.rs:562-575).
// Host arithmetic on a few hundred field elements; no device, no other header of the host.
#pragma once
#include <array>
#include <map>
#include <stdexcept>

#include "fr.hpp"

namespace zkhost {

namespace detail {
// 1 / prod_{m != k} (k - m), k < K: the denominators of the Lagrange basis on the nodes 0 .. K - 1, inverted once per K and thread
inline const FrVec &lagrange_inv_den(size_t K) {
    thread_local std::map<size_t, FrVec> cache;
    FrVec &den = cache[K];
    if (den.empty())
        for (size_t k = 0; k < K; ++k) {
            Fr d = Fr::one();
            for (size_t m = 0; m < K; ++m)
                if (m != k) d *= Fr::from_u64(k) - Fr::from_u64(m);
            den.push_back(d.inverse());
        }
    return den;
}
}  // namespace detail

// the polynomial of degree K - 1 through (k, e[k]), k < K, at x (Lagrange), K >= 2
inline Fr round_poly_nodes(const Fr *e, size_t K, const Fr &x) {
    if (K < 2) throw std::invalid_argument("round_poly_nodes: at least two nodes");
    const FrVec &den = detail::lagrange_inv_den(K);
    Fr acc = Fr::zero();
    for (size_t k = 0; k < K; ++k) {
        Fr num = Fr::one();
        for (size_t m = 0; m < K; ++m)
            if (m != k) num *= x - Fr::from_u64(m);
        acc += e[k] * num * den[k];
    }
    return acc;
}
template <size_t K>
inline Fr round_poly_nodes(const std::array<Fr, K> &e, const Fr &x) {
    return round_poly_nodes(e.data(), K, x);
}

// The chain over rows[i] = the K values of round i (a std::array<Fr, K> or an FrVec each), one challenge per round.  false at the
// first round whose p(0) + p(1) misses its target; true with *last = p_{n-1}(r_{n-1}) (claimed itself for no rounds) otherwise.
// A count that does not fit -- the caller's "malformed" case, checked there -- throws std::invalid_argument.
template <class Rows>
inline bool round_chain(const Rows &rows, size_t K, const FrVec &chal, const Fr &claimed, Fr *last) {
    if (K < 2) throw std::invalid_argument("round_chain: at least two nodes");
    if (rows.size() != chal.size()) throw std::invalid_argument("round_chain: one challenge per round");
    Fr target = claimed;
    for (size_t i = 0; i < rows.size(); ++i) {
        if (rows[i].size() != K) throw std::invalid_argument("round_chain: a round that does not hold K values");
        if (rows[i][0] + rows[i][1] != target) return false;
        target = round_poly_nodes(rows[i].data(), K, chal[i]);
    }
    if (last) *last = target;
    return true;
}

}  // namespace zkhost
