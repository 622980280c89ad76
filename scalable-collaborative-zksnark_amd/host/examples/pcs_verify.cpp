// pcs_verify -- the reference's should_commit_and_open (dist-primitive/src/dpoly_comm.rs:502-531) on the compiled host: a structured
// parameter set (PolynomialCommitmentCub::new, :37-67) and its powers_of_g2 (g2 * s_i by zk_msm_g2), commit / open of seeded
// polynomials, and PolynomialCommitment::verify (:466-484) on the device through zk_pcs_verify_batch -- for the honest opening and
// for five mutations of it.  One verdict line per case; exit 0 when every honest opening is accepted and every mutation rejected.
// No Python and no oracle in the loop; without a GPU it refuses (this host has no CPU fallback).
//
//     bin/pcs_verify [--n NVARS] [--seed SEED]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "zkhost/dist_primitive.hpp"
#include "zkhost/hyperplonk.hpp"
#include "zkhost/pcs_vk.hpp"

using namespace zkhost;

int main(int argc, char **argv) {
    size_t n = 6;
    uint64_t seed = 502;
    for (int i = 1; i + 1 < argc; i += 2) {
        std::string k = argv[i];
        if (k == "--n") n = std::strtoull(argv[i + 1], nullptr, 10);
        else if (k == "--seed") seed = std::strtoull(argv[i + 1], nullptr, 10);
    }
    int ngpu = zk_device_count();
    if (ngpu <= 0) {
        std::fprintf(stderr, "pcs_verify: no GPU visible -- this host has no CPU fallback (zk_device_count = %d)\n", ngpu);
        return 2;
    }
    try {
        Ctx be(0);
        SplitMix64 rng(seed);
        const FrVec s = rng.fr_vec(n), u = rng.fr_vec(n);
        const FrVec poly = rng.fr_vec(size_t(1) << n), poly2 = rng.fr_vec(size_t(1) << n);
        PolynomialCommitmentCub cub = PolynomialCommitmentCub::make(be, s);
        const PowersOfG &pg = cub.mature();
        const size_t len = size_t(1) << n;
        const G1 C = commit(be, pg, be.to_device(poly), len), C2 = commit(be, pg, be.to_device(poly2), len);
        const Opening op = open(be, pg, be.to_device(poly), len, u);

        std::shared_ptr<PcsVk> vk = make_pcs_vk(be, s);  // powers_of_g2 = [g2, s_0 g2, ..., s_{n-1} g2] (dpoly_comm.rs:59-62)

        // the generator g1 = powers_of_g[0][0] as a normalised Jacobian point, infinity as (1, 1, 0)
        uint64_t g1a[12];
        be.check(zk_srs_download(be.handle(), pg[0]->handle(), g1a));
        G1 g1{}, inf{};
        std::memcpy(g1.data(), g1a, 96);
        std::memcpy(g1.data() + 12, Fq::one().v, 48);
        std::memcpy(inf.data(), Fq::one().v, 48);
        std::memcpy(inf.data() + 6, Fq::one().v, 48);

        struct Case {
            std::string name;
            G1 C;
            Fr v;
            G1Vec pf;
            FrVec pt;
            bool expect;
        };
        std::vector<Case> cases;
        cases.push_back({"honest", C, op.value, op.proofs, u, true});
        cases.push_back({"value+1", C, op.value + Fr::one(), op.proofs, u, false});
        {
            G1Vec pf = op.proofs;
            pf[n / 2] = be.g1_lincomb_batch(G1Vec{pf[n / 2], g1}, FrVec{Fr{{1, 0, 0, 0}}, Fr{{1, 0, 0, 0}}}, 1)[0];
            cases.push_back({"proof+g1", C, op.value, pf, u, false});
        }
        if (n > 1) cases.push_back({"point_reversed", C, op.value, op.proofs, FrVec(u.rbegin(), u.rend()), false});
        cases.push_back({"other_commitment", C2, op.value, op.proofs, u, false});
        {
            G1Vec pf = op.proofs;
            pf[0] = inf;
            cases.push_back({"proof_at_infinity", C, op.value, pf, u, false});
        }
        G1Vec cs;
        FrVec vs;
        std::vector<G1Vec> pfs;
        std::vector<FrVec> pts;
        for (auto &c : cases) cs.push_back(c.C), vs.push_back(c.v), pfs.push_back(c.pf), pts.push_back(c.pt);
        std::vector<bool> ok = verify_batch(be, *vk, cs, vs, pfs, pts);
        // the single-opening form agrees with the batch
        bool single = verify(be, *vk, C, op.value, op.proofs, u);
        int bad = single == ok[0] ? 0 : 1;
        for (size_t i = 0; i < cases.size(); ++i) {
            std::printf("should_commit_and_open n=%zu %s: %s\n", n, cases[i].name.c_str(), ok[i] ? "accept" : "reject");
            if (ok[i] != cases[i].expect) ++bad;
        }
        std::printf("pcs_verify: %s\n", bad ? "UNEXPECTED VERDICTS" : "all verdicts as expected");
        return bad ? 1 : 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "pcs_verify: %s\n", e.what());
        return 1;
    }
}
