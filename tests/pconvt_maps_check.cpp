// Stand-alone host check of ds-gan_amd/csrc/pconvt_maps.h (built and run by test_pconvt_maps_cpu.py).
// For whole launches of pconvt_ring_kernel it replays, with the kernel's own loops and the header's
// maps, every LDS-DMA item, the convert pass and the MFMA fragment reads on a tagged model of the
// stage, and asserts that
//   * every source range that is not the zero block lies inside its tensor (weights [T][M][K]; the K
//     channel planes of image b at batch stride x_bs) and is 16-byte aligned,
//   * every LDS byte a fragment read or the convert pass touches was written exactly once in the
//     stage, by the item that carries the value the register-staged kernel would have put there,
//   * the stages and the image fit the declared LDS (160 KB).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pconvt_maps.h"

using namespace dsg;

static long g_checks = 0, g_fail = 0;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    ++g_checks;                                            \
    if (!(cond)) {                                         \
      if (++g_fail <= 20) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                                      \
  } while (0)

static const long ZERO = -2, UNSET = -1;

struct Shape { int N, K, M, Hi, Wi, KS; long x_pad; bool all; };

template <int KS, int BM>
static void sweep(const Shape& s) {
  using R = PtRing<KS, BM>;
  constexpr int NW = R::NW, TH = R::TH, TW = R::TW, BN = TH * TW;
  constexpr int WMW = BM / 32, WNW = NW / WMW, NT = (BN / 32) / WNW;
  constexpr int NA = (R::A_PIECES + NW - 1) / NW, NP = (R::P_PIECES + NW - 1) / NW;
  static_assert(R::LDS_BYTES <= 160 * 1024 && R::LDS_BYTES == 2 * R::STAGE + R::IMG_BYTES, "LDS");
  static_assert(R::STAGE % 16 == 0 && R::A_BYTES % 1024 == 0, "stage alignment");
  const int HWi = s.Hi * s.Wi, nkb = s.K / 32;
  const long x_bs = (long)s.K * HWi + s.x_pad, w_elems = (long)R::T * s.M * s.K;
  const int tiles_w = (s.Wi + 15) / 16, tiles_h = (s.Hi + 7) / 8, mt = (s.M + BM - 1) / BM;
  const int IMG_ELEMS = R::IMG_BYTES / 2;
  std::vector<long> a_tag(R::A_ITEMS), p_tag(R::P_BYTES / 4), i_tag(IMG_ELEMS);
  std::vector<int> a_cnt(R::A_ITEMS), p_cnt(R::P_BYTES / 4), i_cnt(IMG_ELEMS);

  for (int b = 0; b < s.N; ++b) {
    if (!s.all && b != 0 && b != s.N - 1) continue;
    for (int th = 0; th < tiles_h; ++th)
      for (int tw = 0; tw < tiles_w; ++tw)
        for (int m_t = 0; m_t < mt; ++m_t)
          for (int kb = 0; kb < nkb; ++kb) {
            if (!s.all && kb != 0 && kb != nkb - 1) continue;
            const int m0 = m_t * BM, i0 = th * TH, j0 = tw * TW;
            a_tag.assign(a_tag.size(), UNSET); p_tag.assign(p_tag.size(), UNSET); i_tag.assign(i_tag.size(), UNSET);
            a_cnt.assign(a_cnt.size(), 0); p_cnt.assign(p_cnt.size(), 0); i_cnt.assign(i_cnt.size(), 0);
            // ---- the LDS-DMA issue loops of the kernel ----
            for (int wave = 0; wave < NW; ++wave)
              for (int lane = 0; lane < 64; ++lane) {
                for (int i = 0; i < NA; ++i) {
                  const int p = wave + NW * i;
                  if (p >= R::A_PIECES) continue;
                  const int it = p * 64 + lane;
                  const int aoff = (int)R::a_src(it, m0, s.M, s.K, 0);
                  CHECK(R::a_src(it, m0, s.M, s.K, 0) == (long)aoff, "weight offset overflows int");
                  long src = ZERO;
                  if (aoff >= 0) {
                    src = (long)kb * 32 + aoff;
                    CHECK(src >= 0 && src + 8 <= w_elems && src % 8 == 0, "weight src %ld of %ld (item %d)", src, w_elems, it);
                  }
                  const int byte = p * 1024 + lane * 16;
                  CHECK(byte + 16 <= R::A_BYTES, "weight LDS byte %d", byte);
                  a_tag[byte / 16] = src; a_cnt[byte / 16]++;
                }
                for (int i = 0; i < NP; ++i) {
                  const int p = wave + NW * i;
                  if (p >= R::P_PIECES) continue;
                  const int q = p * 64 + lane;
                  const long po = R::p_src(q, i0, j0, s.Hi, s.Wi);
                  const int poff = (int)po;
                  CHECK(po == (long)poff, "patch offset overflows int");
                  long src = ZERO;
                  if (poff >= 0) {
                    const long in_img = (long)kb * 32 * HWi + poff;
                    CHECK(in_img >= 0 && in_img + 4 <= (long)s.K * HWi, "patch src %ld outside the image's %ld floats", in_img, (long)s.K * HWi);
                    src = (long)b * x_bs + in_img;
                    CHECK(src % 4 == 0 && src + 4 <= (long)s.N * x_bs, "patch src %ld alignment / tensor end", src);
                    // a 4-float item never straddles two image rows
                    CHECK((poff % HWi) / s.Wi == (poff % HWi + 3) / s.Wi, "patch item straddles rows");
                  }
                  const int byte = R::A_BYTES + p * 1024 + lane * 16;
                  CHECK(byte + 16 <= R::STAGE, "patch LDS byte %d", byte);
                  for (int e = 0; e < 4; ++e) {
                    const int f = (byte - R::A_BYTES) / 4 + e;
                    p_tag[f] = src == ZERO ? ZERO : src + e; p_cnt[f]++;
                  }
                }
              }
            // ---- A fragment reads ----
            for (int tap = 0; tap < R::T; ++tap)
              for (int row = 0; row < BM; ++row)
                for (int ls = 0; ls < 4; ++ls) {
                  const int byte = R::a_frag_byte(tap, row, ls);
                  CHECK(byte >= 0 && byte + 16 <= R::A_BYTES && byte % 16 == 0, "A fragment byte %d", byte);
                  const int m = m0 + row;
                  const long want = m < s.M ? ((long)tap * s.M + m) * s.K + kb * 32 + ls * 8 : ZERO;
                  CHECK(a_cnt[byte / 16] == 1, "A unit %d written %d times", byte / 16, a_cnt[byte / 16]);
                  CHECK(a_tag[byte / 16] == want, "A fragment (tap %d row %d slot %d): %ld, want %ld", tap, row, ls, a_tag[byte / 16], want);
                }
            // ---- convert pass ----
            for (int it = 0; it < R::C_ITEMS; ++it) {
              const auto c = R::c_item(it);
              CHECK(c.cg >= 0 && c.cg < 4 && c.pr >= 0 && c.pr < R::PH && c.pc >= 0 && c.pc < R::PW, "convert item %d", it);
              CHECK(R::img_elem(c.pr, c.pc, c.cg * 8) % 8 == 0, "image write alignment");
              for (int e = 0; e < 8; ++e) {
                const int byte = R::p32_byte(c.cg * 8 + e, c.pr, c.pc);
                CHECK(byte >= R::A_BYTES && byte + 4 <= R::STAGE && byte % 4 == 0, "fp32 patch byte %d", byte);
                const int f = (byte - R::A_BYTES) / 4;
                CHECK(p_cnt[f] == 1, "fp32 patch float %d written %d times", f, p_cnt[f]);
                const int el = R::img_elem(c.pr, c.pc, c.cg * 8 + e);
                CHECK(el >= 0 && el < IMG_ELEMS, "image element %d", el);
                i_tag[el] = p_tag[f]; i_cnt[el]++;
              }
            }
            // ---- B fragment reads (pconvt_kernel's pbase arithmetic) ----
            for (int wn = 0; wn < WNW; ++wn)
              for (int j = 0; j < NT; ++j)
                for (int lane = 0; lane < 64; ++lane) {
                  const int lr = lane & 31, lh = lane >> 5;
                  const int n = (wn * NT + j) * 32 + lr;
                  const int pbase = ((n / TW) * R::PWP + (n % TW)) * R::STR + lh * 8;
                  for (int sh = 0; sh < R::NSH; ++sh)
                    for (int sw = 0; sw < R::NSH; ++sw)
                      for (int ks = 0; ks < 2; ++ks)
                        for (int e = 0; e < 8; ++e) {
                          const int el = pbase + (sh * R::PWP + sw) * R::STR + ks * 16 + e;
                          CHECK(el >= 0 && el < IMG_ELEMS, "B fragment element %d", el);
                          const int ch = ks * 16 + lh * 8 + e;
                          const int ih = i0 + R::DMIN + n / TW + sh, iw = j0 + R::DMIN + n % TW + sw;
                          const bool in = ih >= 0 && ih < s.Hi && iw >= 0 && iw < s.Wi;
                          const long want = in ? (long)b * x_bs + ((long)kb * 32 + ch) * HWi + (long)ih * s.Wi + iw : ZERO;
                          CHECK(i_cnt[el] == 1, "image element %d written %d times", el, i_cnt[el]);
                          CHECK(i_tag[el] == want, "B fragment (pixel %d shift %d,%d ch %d): %ld, want %ld", n, sh, sw, ch, i_tag[el], want);
                        }
                }
          }
  }
}

int main() {
  // (N, K, M, Hi, Wi, KS, extra batch stride, every image and K block)
  const Shape shapes[] = {
      // the cases of tests/test_pconvt_ring_gpu.py
      {1, 32, 64, 8, 16, 3, 0, true},   {2, 64, 64, 16, 32, 3, 0, true}, {1, 96, 96, 8, 16, 3, 0, true},
      {1, 64, 32, 12, 20, 3, 0, true},  {2, 64, 32, 16, 16, 4, 0, true}, {1, 96, 64, 8, 20, 4, 0, true},
      {2, 64, 64, 16, 32, 3, 32 * 16 * 32, true}, {2, 64, 32, 16, 16, 4, 64 * 16 * 16, true},
      {2, 32, 40, 4, 4, 3, 4, true},    {1, 32, 8, 20, 36, 4, 0, true},
      // the step's shapes (batch 16): first / last image, first / last K block
      {16, 128, 64, 128, 128, 3, 0, false}, {16, 256, 128, 64, 64, 3, 0, false}, {16, 1024, 512, 16, 16, 3, 0, false},
      {16, 512, 256, 32, 32, 3, 0, false},  {16, 256, 128, 16, 16, 3, 0, false}, {16, 128, 64, 64, 64, 3, 0, false},
      {16, 128, 64, 32, 32, 3, 0, false},   {16, 128, 64, 32, 32, 4, 0, false},  {16, 64, 32, 64, 64, 4, 0, false},
  };
  for (const Shape& s : shapes) {
    if (s.KS == 3) sweep<3, 64>(s);
    else sweep<4, 32>(s);
  }
  std::printf("%s: %ld checks, %ld failed\n", g_fail ? "FAILED" : "OK", g_checks, g_fail);
  return g_fail ? 1 : 0;
}
