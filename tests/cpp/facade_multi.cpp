// The multi-vector apply through the reference-style C++ surface:
// PreconditioningMulti with three residuals against three Preconditioning
// calls on the same object, compared bit for bit.  Inputs come from binary
// files written by tests/test_gpu_multi_rhs.py.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "SeSchwarzPreconditioner.h"

using namespace SE;

template <class T>
static std::vector<T> load(const std::string& path) {
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    size_t n = f.tellg();
    f.seekg(0);
    std::vector<T> v(n / sizeof(T));
    f.read(reinterpret_cast<char*>(v.data()), n);
    return v;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string d = argv[1];
    auto pos = load<SeVec3fSimd>(d + "/pos.bin");
    auto starts = load<int>(d + "/starts.bin");
    auto idx = load<int>(d + "/idx.bin");
    auto diag = load<SeMatrix3f>(d + "/diag.bin");
    auto off = load<SeMatrix3f>(d + "/off.bin");
    const int nV = (int)pos.size();
    constexpr int K = 3;
    std::vector<SeVec3fSimd> r[K], zm[K], zs[K];
    for (int k = 0; k < K; ++k) {
        r[k] = load<SeVec3fSimd>(d + "/r" + std::to_string(k) + ".bin");
        if ((int)r[k].size() != nV) return 3;
        zm[k].resize(nV);
        zs[k].resize(nV);
    }

    SeCsr<int> csr(starts, idx, {});
    SeSchwarzPreconditioner P;
    P.m_positions = pos.data();
    P.m_neighbours = &csr;
    P.AllocatePrecoditioner(nV, 0, 0);
    std::vector<unsigned> efC(1, 0), eeC(1, 0), vfC(nV + 1, 0);
    P.PreparePreconditioner(diag.data(), off.data(), starts.data(), nullptr, nullptr, nullptr, efC.data(), eeC.data(),
                            vfC.data());
    std::printf("stage prepare\n");
    std::fflush(stdout);

    SeVec3fSimd* zp[K];
    const SeVec3fSimd* rp[K];
    for (int k = 0; k < K; ++k) {
        zp[k] = zm[k].data();
        rp[k] = r[k].data();
    }
    P.PreconditioningMulti(zp, rp, K, 3 * nV);
    std::printf("stage multi\n");
    std::fflush(stdout);
    for (int k = 0; k < K; ++k) P.Preconditioning(zs[k].data(), r[k].data(), 3 * nV);
    bool same = true, nonzero = false;
    for (int k = 0; k < K; ++k) {
        same = same && std::memcmp(zm[k].data(), zs[k].data(), (size_t)nV * 16) == 0;
        for (int v = 0; v < nV; ++v) nonzero = nonzero || zm[k][v][0] != 0.f;
    }
    // an aliased output is refused, not computed
    bool refused = false;
    try {
        SeVec3fSimd* bad[K] = {zm[0].data(), zm[0].data(), zm[2].data()};
        P.PreconditioningMulti(bad, rp, K, 3 * nV);
    } catch (const std::runtime_error&) {
        refused = true;
    }
    std::printf("multi_nonzero %d\n", nonzero ? 1 : 0);
    std::printf("multi_alias_refused %d\n", refused ? 1 : 0);
    std::printf("multi_bitwise %d\n", same ? 1 : 0);
    return 0;
}
