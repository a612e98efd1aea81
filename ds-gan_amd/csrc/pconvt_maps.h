// Address maps of the LDS-DMA ring form of pconvt.hip (pconvt_ring_kernel): which 16 bytes of global
// memory every LDS-DMA item copies, where they land in the stage, and where the convert pass and the
// MFMA fragment reads find them again.  Plain inline functions of integers, compiled by hipcc for the
// kernel and by a host C++ compiler for tests/test_pconvt_maps_cpu.py, which sweeps them over whole
// launches before a kernel ever runs them.
//
// One stage holds a 32-channel K block of one workgroup tile (BM output channels x TH x TW grid pixels):
//   [0, A_BYTES)           weights  [tap][row][4 slots of 16 B]; row r keeps its logical slot s (8 of
//                          the 32 channels) at physical slot s ^ ((r >> 2) & 3): an LDS-DMA writes
//                          lane-linear, so the row pitch stays 64 B and the XOR on the SOURCE address
//                          (undone on the fragment read) spreads the 16 rows of a ds_read_b128 group
//                          over the 16 distinct 16-byte bank groups
//   [A_BYTES, STAGE)       fp32 patch [channel][patch row][NI items of 4 floats] as the rows lie in
//                          NCHW, from image column j0 - COFF; items outside the image copy a zero block
// and one bf16 image [PH][PWP][STR] (pconvt_kernel's: pixel-major, 32 channels + 8 pad) is shared by
// the stages: the convert pass rounds a landed fp32 patch into it.
#pragma once

#if defined(__HIPCC__)
#define PTM_HD __host__ __device__ __forceinline__
#else
#define PTM_HD inline
#endif

namespace dsg {

template <int KS, int BM>
struct PtRing {
  static constexpr int T = KS * KS, TH = 8, TW = 16;
  static constexpr int DMIN = KS == 3 ? 0 : -1, NSH = KS == 3 ? 2 : 3;   // PtGeo<KS, 1>
  static constexpr int PH = TH + NSH - 1, PW = TW + NSH - 1, PWP = 32, STR = 40;
  static constexpr int COFF = DMIN < 0 ? 4 : 0;                  // first staged column is j0 - COFF
  static constexpr int NI = (PW - 1 + DMIN + COFF) / 4 + 1;      // 4-float items per patch row
  static constexpr int A_ITEMS = T * BM * 4, A_PIECES = A_ITEMS / 64, A_BYTES = A_ITEMS * 16;
  static constexpr int P_ITEMS = 32 * PH * NI, P_PIECES = (P_ITEMS + 63) / 64, P_BYTES = P_PIECES * 1024;
  static constexpr int STAGE = A_BYTES + P_BYTES;
  static constexpr int IMG_BYTES = PH * PWP * STR * 2;
  static constexpr int LDS_BYTES = 2 * STAGE + IMG_BYTES;
  static constexpr int C_ITEMS = PH * PW * 4;                    // convert items: (8-channel group, pixel)
  static constexpr int NW = BM / 32 * 4;                         // waves: BM / 32 along M x 4 along pixels
  static_assert(A_ITEMS % 64 == 0 && BM % 16 == 0, "an LDS-DMA piece is 16 whole weight rows");
  static_assert(DMIN + COFF >= 0, "left halo inside the first item");

  // ---- weights: item (16 B of the stage's A region, in LDS order) -> source -----------------
  struct AItem { int tap, row, pslot, lslot; };
  static PTM_HD AItem a_item(int it) {
    const int r = it >> 2, row = r % BM, p = it & 3;
    return AItem{r / BM, row, p, p ^ ((row >> 2) & 3)};
  }
  // element offset into Wb [T][M][K] of the item's 8 values, -1: row m0 + row >= M (zero block)
  static PTM_HD long a_src(int it, int m0, int M, int K, int k0) {
    const AItem a = a_item(it);
    const int m = m0 + a.row;
    return m < M ? ((long)a.tap * M + m) * K + k0 + a.lslot * 8 : -1;
  }
  // LDS byte (within the stage) of the 8 values k = 8 lslot .. 8 lslot + 7 of weight row `row`, tap `tap`
  static PTM_HD int a_frag_byte(int tap, int row, int lslot) {
    return ((tap * BM + row) * 4 + (lslot ^ ((row >> 2) & 3))) * 16;
  }

  // ---- fp32 patch: item q (16 B of the stage's patch region, in LDS order) -> source ---------
  struct PItem { int c, pr, wi; };
  static PTM_HD PItem p_item(int q) {
    const int c = q / (PH * NI), rem = q - c * (PH * NI);
    return PItem{c, rem / NI, rem % NI};
  }
  // float offset, from channel k0 of the image, of the item's 4 floats; -1: outside (zero block).
  // Wi % 4 == 0 and j0 % 16 == 0, so an item is wholly inside or wholly outside a row.
  static PTM_HD long p_src(int q, int i0, int j0, int Hi, int Wi) {
    if (q >= P_ITEMS) return -1;
    const PItem p = p_item(q);
    const int ih = i0 + DMIN + p.pr, iw = j0 - COFF + 4 * p.wi;
    if ((unsigned)ih >= (unsigned)Hi || (unsigned)iw >= (unsigned)Wi) return -1;
    return (long)p.c * Hi * Wi + (long)ih * Wi + iw;
  }
  // LDS byte (within the stage) of the fp32 value of channel c at patch pixel (pr, pc)
  static PTM_HD int p32_byte(int c, int pr, int pc) {
    return A_BYTES + ((c * PH + pr) * NI) * 16 + (pc + DMIN + COFF) * 4;
  }

  // ---- convert pass: item -> (8-channel group, patch pixel); bf16 image ----------------------
  struct CItem { int cg, pr, pc; };
  static PTM_HD CItem c_item(int it) {
    const int cg = it / (PH * PW), pix = it - cg * (PH * PW);
    return CItem{cg, pix / PW, pix % PW};
  }
  // element (16-bit) index into the image of channel c of patch pixel (pr, pc)
  static PTM_HD int img_elem(int pr, int pc, int c) { return (pr * PWP + pc) * STR + c; }
};

}  // namespace dsg
