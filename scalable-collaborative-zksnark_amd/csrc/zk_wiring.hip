// zk_wiring.hip -- the wiring identity of HyperPlonk (the ProductCheck of its PermCheck) as ONE sumcheck; the reference simulates it
// with six independent product sumchecks on six unrelated polynomials (hyperplonk/src/hyperplonk.rs:94-141):
//   K11  wiring sumcheck     F(x) = eq(x) [ v(1,x) - v(x,0) v(x,1) + gamma ( den(x) h(x) - num(x) ) ], degree 3 per variable:
//                            four evaluations of the round polynomial (t = 0 .. 3) per round, seven tables folded
//                            (eq, v1x, vx0, vx1, h, num, den).
// v is the product tree of h = num / den (zk_product_tree: tree[0..N) = h, tree[N + j] = tree[2j] tree[2j+1], tree[2N-1] = 0); with
// index bit 0 the TOP bit, v(0,x) = tree[x], v(1,x) = tree[N + x], v(x,0) = tree[2x], v(x,1) = tree[2x + 1].
//
// Conventions of zk_fr.hip / zk_gate.hip: Fr in Montgomery form, 32-byte AoS elements, round i binds the TOP index bit, inputs are
// never written, all sums are exact modular sums.
//
// The sumcheck is the preset-challenge engine of zk_fused.cuh over WireKind (zk_gate.cuh).  The four views are read straight out of
// the tree -- h and v1x are its halves, vx0 and vx1 every other element from its base / one element on (shift 1 of FsIn) -- so nobody
// makes deinterleaved copies; later passes read the folded ping-pong tables.  Per index pair and t four multiplications (three reduced
// ones inside the bracket, the product with eq left as an integer), with the seven folds 7 + 4 x 4 = 23 per index pair.
#include "zk_fused.cuh"

namespace zk {

// ---------------------------------------------------------------------------------------
// host driver
// ---------------------------------------------------------------------------------------
int sumcheck_wiring(zk_ctx* ctx, const void* d_eq, const void* d_tree, const void* d_num, const void* d_den, size_t N, const uint64_t* h_gamma,
                    const uint64_t* h_chal, uint64_t* h_out_evals, uint64_t* h_last) {
    return run_preset<WireKind>(ctx, "zk_sumcheck_wiring", "N = ", bind_wiring(d_eq, d_tree, d_num, d_den, N, h_gamma), N, h_chal, h_out_evals, h_last);
}

}  // namespace zk
