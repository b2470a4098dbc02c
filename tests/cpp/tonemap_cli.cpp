// C++ caller of me::amd::tonemap16 and of the loop's 16-bit entry
// (include/MotionEstimationAMD/motion_estimation_amd.hpp) -- tests only.
//
//   tonemap_cli <in.bin> <out.bin>
// in.bin: int32 {width, height, step (elements), lo_ppm, hi_ppm, min_span,
// alpha_q8}, then the image (height rows of `step` uint16).  out.bin: the 8-bit
// image (width * height bytes, dense), then one byte per WindowedStereoVO check:
// [0] process16 without setToneMap threw, [1] setToneMap with bad parameters
// threw, [2] setToneMap / clearToneMap with good ones did not.
#include <cstdint>
#include <cstdio>
#include <vector>
#include "MotionEstimationAMD/motion_estimation_amd.hpp"

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: tonemap_cli <in.bin> <out.bin>\n");
    return 2;
  }
  std::FILE* fh = std::fopen(argv[1], "rb");
  if (!fh) {
    std::perror(argv[1]);
    return 2;
  }
  int32_t hdr[7];
  bool ok = std::fread(hdr, 4, 7, fh) == 7;
  ok = ok && hdr[0] > 0 && hdr[1] > 0 && hdr[2] >= hdr[0];
  std::vector<uint16_t> img;
  if (ok) {
    img.resize((size_t)hdr[2] * hdr[1]);
    ok = std::fread(img.data(), 2, img.size(), fh) == img.size();
  }
  std::fclose(fh);
  if (!ok) {
    std::fprintf(stderr, "tonemap_cli: short or malformed input\n");
    return 2;
  }
  try {
    const me::amd::ImageView16 v{img.data(), hdr[1], hdr[0], hdr[2]};
    me::amd::ToneMapParams p;
    p.loPpm = hdr[3];
    p.hiPpm = hdr[4];
    p.minSpan = hdr[5];
    p.alphaQ8 = hdr[6];
    const std::vector<uint8_t> out = me::amd::tonemap16(v, p);
    // the loop's switch, on a loop that never sees a keyframe
    uint8_t checks[3] = {0, 0, 0};
    {
      me::WindowedStereoVO::Config cfg;  // (the default configuration)
      me::amd::Context ba(0), front(0);
      me::WindowedStereoVO vo(ba, front, cfg, 0);
      const std::vector<uint16_t> z((size_t)cfg.width * cfg.height, 0);
      const me::amd::ImageView16 zv{z.data(), cfg.height, cfg.width, cfg.width};
      try {
        vo.process16(0, zv, zv);
      } catch (const std::exception&) {
        checks[0] = 1;
      }
      me::amd::ToneMapParams bad;
      bad.alphaQ8 = 0;
      try {
        vo.setToneMap(bad);
      } catch (const std::exception&) {
        checks[1] = 1;
      }
      vo.setToneMap(p);
      vo.clearToneMap();
      checks[2] = 1;
    }
    std::FILE* fo = std::fopen(argv[2], "wb");
    if (!fo) {
      std::perror(argv[2]);
      return 2;
    }
    ok = std::fwrite(out.data(), 1, out.size(), fo) == out.size() && std::fwrite(checks, 1, 3, fo) == 3;
    ok = (std::fclose(fo) == 0) && ok;
    if (!ok) {
      std::fprintf(stderr, "tonemap_cli: write failed\n");
      return 2;
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "tonemap_cli: %s\n", e.what());
    return 1;
  }
  return 0;
}
