// The three kernels of csrc/spectrum.hip on the host: every phase between two barriers is a __host__ __device__ function, and this
// program runs a launch workgroup by workgroup, phase by phase, over the 256 threads — with the LDS arrays, the workspace and the
// outputs as exactly sized heap blocks, so that a host sanitizer sees any index past an end before a kernel ever runs on a GPU:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -I wt-pse-code_amd/wtpse_hip/csrc -I include \
//         -Xarch_host -fsanitize=address,undefined tools/probe/spectrum_host.hip -o spectrum_host
//   ./spectrum_host in.bin out.bin
// in.bin: int32 N, S, b | img uint8 [N][S][S][3] | partner int32 [N] | lam float [N] | twiddle float [S][2];
// out.bin: uint8 [N][S][S][3] | float [N][S][S][3].  It calls nothing of the HIP runtime: no GPU is needed.
// tools/probe/spectrum_host.py builds it, writes in.bin from seeded pictures, runs it and compares out.bin with the specification.
#include "spectrum.hip"
#include <cstdio>
#include <cstdlib>
#include <vector>

template <int S, int KS> struct Wg {
  std::vector<float> re, im, twr, twi;
  AmixLds L;
  Wg() : re(AmixShared<S, KS>::FLOATS), im(AmixShared<S, KS>::FLOATS), twr(S), twi(S) { L = {re.data(), im.data(), twr.data(), twi.data()}; }
};
#define FOR_T for (int tid = 0; tid < 256; ++tid) { const int g = tid / AmixGeo<S>::TG, j = tid % AmixGeo<S>::TG; const int item = blk * AmixGeo<S>::NG + g; (void)item; (void)j;
#define END_T }

template <int S, int KS, int K, bool INV> void fft(const AmixLds& L) {
  int p = 0, Ns = 1;
  for (int q = 0; q < AmixPasses<S>::R4; ++q) {
    for (int tid = 0; tid < 256; ++tid) amix_pass4<S, KS, K, INV>(L, tid / AmixGeo<S>::TG, tid % AmixGeo<S>::TG, Ns, p);
    p ^= 1; Ns *= 4;
  }
  if (AmixPasses<S>::R2) for (int tid = 0; tid < 256; ++tid) amix_pass2<S, KS, K, INV>(L, tid / AmixGeo<S>::TG, tid % AmixGeo<S>::TG, p);
}

template <int S> void run(const AmixArgs& A) {
  constexpr int NG = AmixGeo<S>::NG;
  const int pairs = (A.N * (S / 2) + NG - 1) / NG, cols = (A.N * 3 * (A.b + 1) + NG - 1) / NG;
  for (int blk = 0; blk < pairs; ++blk) {
    Wg<S, 3> w; const AmixLds& L = w.L;
    FOR_T amix_load_twiddle<S>(A, L, tid); END_T
    FOR_T amix_rows_load<S>(A, L, item, g, j); END_T
    fft<S, 3, 3, false>(L);
    FOR_T amix_rows_store<S>(A, L, item, g, j); END_T
  }
  for (int blk = 0; blk < cols; ++blk) {
    Wg<S, 2> w; const AmixLds& L = w.L;
    FOR_T amix_load_twiddle<S>(A, L, tid); END_T
    FOR_T amix_cols_load<S>(A, L, item, g, j); END_T
    fft<S, 2, 2, false>(L);
    FOR_T amix_cols_mix<S>(A, L, item, g, j); END_T
    fft<S, 2, 1, true>(L);
    FOR_T amix_cols_store<S>(A, L, item, g, j); END_T
  }
  for (int blk = 0; blk < pairs; ++blk) {
    Wg<S, 3> w; const AmixLds& L = w.L;
    FOR_T amix_load_twiddle<S>(A, L, tid); END_T
    FOR_T amix_finish_load<S>(A, L, item, g, j); END_T
    fft<S, 3, 3, true>(L);
    FOR_T amix_finish_store<S>(A, L, item, g, j); END_T
  }
}

template <class T> std::vector<T> rd(FILE* f, size_t n) { std::vector<T> v(n); if (fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); } return v; }

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  auto hdr = rd<int>(f, 3);
  const int N = hdr[0], S = hdr[1], b = hdr[2];
  const size_t px = (size_t)N * S * S * 3;
  auto img = rd<unsigned char>(f, px);
  auto partner = rd<int>(f, N);
  auto lam = rd<float>(f, N);
  auto tw = rd<float>(f, 2 * S);
  fclose(f);
  const int nf = wtpse_amix_workspace(N, S, b);
  if (nf < 0) { fprintf(stderr, "refused\n"); return 3; }
  std::vector<float> work(nf), of(px);   // exactly sized: the sanitizer sees any index past the end
  std::vector<unsigned char> o8(px);
  AmixArgs A;
  A.img = img.data(); A.partner = partner.data(); A.lam = lam.data(); A.twiddle = tw.data(); A.out_u8 = o8.data(); A.out_f32 = of.data();
  A.spec = work.data(); A.corr = work.data() + nf / 2; A.N = N; A.b = b;
  switch (S) { case 32: run<32>(A); break; case 64: run<64>(A); break; case 128: run<128>(A); break; case 256: run<256>(A); break; default: run<512>(A); }
  FILE* o = fopen(argv[2], "wb");
  fwrite(o8.data(), 1, px, o); fwrite(of.data(), 4, px, o); fclose(o);
  return 0;
}
