// C++ test of the opening mirror (halo2-pse_amd/host/halo2hip.hpp: arithmetic::eval_polynomial / kate_division and
// poly::kzg::multiopen's GWC and SHPLONK over the engine).  Needs an MI355X.  tests/test_opening.py writes the input and compares the
// output with its Python restatement.
//   usage: test_opening_mirror <in> <out>
//   in (u64 words): k, n_polys, the polynomials (2^k x 4 each), n_sets, per set: n_points, n_columns, the points (x 4), per column
//                   its polynomial index and its evaluations at the points (x 4); then y, v, u (x 4)
//   out: GWC's witnesses (per point in order of first use, polynomials by index), SHPLONK's h_x, SHPLONK's final quotient
#include <cstdio>
#include <fstream>
#include <map>
#include <vector>

#include "../../halo2-pse_amd/host/halo2hip.hpp"

using namespace halo2_proofs;
using namespace halo2_proofs::poly;

struct Reader {
    std::vector<uint64_t> w;
    size_t at = 0;
    uint64_t word() { return w.at(at++); }
    Fr fr() {
        Fr f;
        for (int i = 0; i < 4; i++) f.l[i] = word();
        return f;
    }
};

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s <in> <out>\n", argv[0]);
        return 2;
    }
    Reader r;
    {
        std::ifstream f(argv[1], std::ios::binary | std::ios::ate);
        r.w.resize(size_t(f.tellg()) / 8);
        f.seekg(0);
        f.read((char*)r.w.data(), std::streamsize(r.w.size() * 8));
    }
    const uint32_t k = uint32_t(r.word());
    const size_t n = size_t(1) << k, n_polys = r.word();
    std::vector<Polynomial<Coeff>> polys(n_polys);
    for (auto& p : polys)
        for (size_t i = 0; i < n; i++) p.values.push_back(r.fr());
    std::vector<kzg::multiopen::RotationSet> sets(r.word());
    std::vector<Fr> order;                       // GWC: points in order of first use
    std::vector<std::map<size_t, Fr>> at_point;  // ... and the polynomials queried there, by index
    for (auto& set : sets) {
        const size_t n_points = r.word(), n_cols = r.word();
        for (size_t t = 0; t < n_points; t++) set.points.push_back(r.fr());
        for (size_t c = 0; c < n_cols; c++) {
            const size_t j = r.word();
            std::vector<Fr> evals;
            for (size_t t = 0; t < n_points; t++) evals.push_back(r.fr());
            set.commitments.push_back({&polys.at(j), evals});
        }
        for (size_t t = 0; t < n_points; t++) {
            size_t g = 0;
            while (g < order.size() && order[g] != set.points[t]) g++;
            if (g == order.size()) {
                order.push_back(set.points[t]);
                at_point.emplace_back();
            }
            for (auto& c : set.commitments) at_point[g][size_t(c.first - polys.data())] = c.second[t];
        }
    }
    const Fr y = r.fr(), v = r.fr(), u = r.fr();

    std::vector<kzg::multiopen::PointQueries> groups;
    for (size_t g = 0; g < order.size(); g++) {
        kzg::multiopen::PointQueries pq{order[g], {}};
        for (auto& q : at_point[g]) pq.queries.push_back({&polys[q.first], q.second});
        groups.push_back(pq);
    }
    int failures = 0;
    // the engine's evaluations agree with the evaluations the input carries
    for (auto& pq : groups)
        for (auto& q : pq.queries)
            if (arithmetic::eval_polynomial(q.first->values, pq.point) != q.second) failures++;
    auto witnesses = kzg::multiopen::gwc_witnesses(groups, v);
    bool squeezed = false;
    auto sh = kzg::multiopen::shplonk(sets, y, v, [&](const Polynomial<Coeff>& h_x) {
        squeezed = h_x.len() == n;  // u is drawn once h_x exists
        return u;
    });
    if (!squeezed) failures++;
    // kate_division against the witness of the first point: the same division of the same combination
    {
        std::vector<Fr> a(n, Fr::zero());
        const auto pw = arithmetic::powers(v, groups[0].queries.size());
        Fr e = Fr::zero();
        for (size_t i = 0; i < groups[0].queries.size(); i++) {
            for (size_t t = 0; t < n; t++) a[t] = a[t] + pw[i] * groups[0].queries[i].first->values[t];
            e = e + pw[i] * groups[0].queries[i].second;
        }
        a[0] = a[0] - e;
        if (arithmetic::kate_division(a, groups[0].point) != witnesses[0].values) failures++;
    }
    std::ofstream out(argv[2], std::ios::binary);
    for (auto& w : witnesses) out.write((const char*)w.values.data(), std::streamsize(w.len() * 32));
    out.write((const char*)sh.h_x.values.data(), std::streamsize(sh.h_x.len() * 32));
    out.write((const char*)sh.final_poly.values.data(), std::streamsize(sh.final_poly.len() * 32));
    if (failures) std::printf("FAIL: %d checks\n", failures);
    return failures ? 1 : 0;
}
