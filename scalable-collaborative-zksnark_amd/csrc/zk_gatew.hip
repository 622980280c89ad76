// zk_gatew.hip -- the WIDE Plonk gate as one ZeroCheck sumcheck.  With N = 2^mu rows, six selectors and the three wires
//   W(x) = eq(x) [ qL a + qR b + qM a b + qH a^5 - qO c + qC + in ],
//   K14  wide gate sumcheck   degree 7 per variable (qH a^5 is degree 6, eq adds one): EIGHT evaluations of the round polynomial
//                             (t = 0 .. 7) per round, eleven tables folded (eq, qL, qR, qM, qO, qC, qH, a, b, c, in).
// A constant selector, separate weights of the two additive wires, an output selector and a fifth-power term: an S-box row
// c = a^5 + const (Poseidon, Rescue) is ONE row, and the sumcheck prover pays for the degree with evaluations, not with a larger FFT.
//
// Conventions of zk_perm3.hip: Fr in Montgomery form, 32-byte AoS elements, round i binds the TOP index bit, inputs are never
// written, all sums are exact modular sums.  The sumcheck is the preset-challenge engine of zk_fused.cuh over GatewKind (zk_gate.cuh).
// Per index pair and t ten multiplications (nine reduced ones inside the bracket, the product with eq left as an integer), with the
// eleven folds 11 + 8 x 10 = 91 per index pair.  Eleven tables of 512 elements would be 176 KiB, more than the CU's 160 KiB of LDS:
// the hand-over is at most kGatewLocalMax = 256 elements (88 KiB).
//
// Registers of the pass: eleven (value, difference) pairs are 176 VGPRs and eight 17-limb sums 136 more, so it is compiled for one
// wave per SIMD (the 264 .. 512 register bracket) and launched with one workgroup per CU.  It does not spill.
#include "zk_fused.cuh"

namespace zk {

int sumcheck_gate_wide(zk_ctx* ctx, const void* const* d_tabs, size_t len, const uint64_t* h_chal, uint64_t* h_out_evals, uint64_t* h_last) {
    return run_preset<GatewKind>(ctx, "zk_sumcheck_gate_wide", "table length ", bind_gate_wide(d_tabs), len, h_chal, h_out_evals, h_last);
}

}  // namespace zk
