// imh::EkfLoop::step (immesh_amd/csrc/ekf_host.hpp, the host loop's 18-state update) as a stand-alone program, so that tests/test_ekf_cpu.py can put
// the product's own code against the long-double checker -- and run it under -fsanitize=address,undefined -- without a device or an interpreter.
//   ekf_host_step IN OUT
// IN:  records of 417 raw doubles: HTH 36, HTz 6, prior 24, iterate 24, P 324, pass index, rematch count on entry, max_iter.
// OUT: records of 352 raw doubles: iterate' 24, stop, rematch count on exit, singular, pose_block_usable(P), covariance 324 (the posterior at a
//      stop, P otherwise).
#include <cstdio>
#include <vector>

#include "ekf_host.hpp"

static const int N_IN = 36 + 6 + 24 + 24 + 324 + 3, N_OUT = 24 + 4 + 324;

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    std::FILE* fi = std::fopen(argv[1], "rb");
    std::FILE* fo = std::fopen(argv[2], "wb");
    if (!fi || !fo) { std::fprintf(stderr, "cannot open files\n"); return 2; }
    std::vector<double> in(N_IN), out(N_OUT);
    int n = 0;
    while (std::fread(in.data(), sizeof(double), N_IN, fi) == (size_t)N_IN) {
        const double *HTH = in.data(), *HTz = HTH + 36, *prior24 = HTz + 6, *state24 = prior24 + 24, *P = state24 + 24;
        const int it = (int)P[324], rematch = (int)P[325], max_iter = (int)P[326];
        std::vector<double> full(348);
        imh::State prior, st;
        std::memcpy(full.data(), prior24, 24 * 8); std::memcpy(full.data() + 24, P, 324 * 8);
        imh::load_state(full.data(), prior);
        std::memcpy(full.data(), state24, 24 * 8);
        imh::load_state(full.data(), st);
        imh::EkfLoop loop;
        loop.rematch_num = rematch;
        const bool stop = loop.step(HTH, HTz, prior, st, it, max_iter);
        imh::store_state(st, full.data());
        std::memcpy(out.data(), full.data(), 24 * 8);
        out[24] = stop ? 1.0 : 0.0; out[25] = (double)loop.rematch_num; out[26] = loop.singular ? 1.0 : 0.0; out[27] = imh::pose_block_usable(P) ? 1.0 : 0.0;
        std::memcpy(out.data() + 28, full.data() + 24, 324 * 8);
        n++;
        if (std::fwrite(out.data(), sizeof(double), N_OUT, fo) != (size_t)N_OUT) { std::fprintf(stderr, "short write\n"); return 2; }
    }
    std::fclose(fi);
    if (std::fclose(fo) != 0) return 2;
    std::printf("%d steps\n", n);
    return 0;
}
