// C++ caller of me::amd::clahe
// (include/MotionEstimationAMD/motion_estimation_amd.hpp) -- tests only.
//
//   clahe_cli <in.bin> <out.bin>
// in.bin: int32 {width, height, step, tiles_x, tiles_y}, double clip_limit,
// the image (height rows of `step` bytes).  out.bin: the equalised image
// (width * height bytes, dense), then the tiles_y * tiles_x * 256 table bytes.
#include <cstdint>
#include <cstdio>
#include <vector>
#include "MotionEstimationAMD/motion_estimation_amd.hpp"

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: clahe_cli <in.bin> <out.bin>\n");
    return 2;
  }
  std::FILE* fh = std::fopen(argv[1], "rb");
  if (!fh) {
    std::perror(argv[1]);
    return 2;
  }
  int32_t hdr[5];
  double clip = 0;
  bool ok = std::fread(hdr, 4, 5, fh) == 5 && std::fread(&clip, 8, 1, fh) == 1;
  ok = ok && hdr[0] > 0 && hdr[1] > 0 && hdr[2] >= hdr[0];
  std::vector<uint8_t> img;
  if (ok) {
    img.resize((size_t)hdr[2] * hdr[1]);
    ok = std::fread(img.data(), 1, img.size(), fh) == img.size();
  }
  std::fclose(fh);
  if (!ok) {
    std::fprintf(stderr, "clahe_cli: short or malformed input\n");
    return 2;
  }
  try {
    const me::amd::ImageView v{img.data(), hdr[1], hdr[0], hdr[2]};
    std::vector<uint8_t> lut;
    const std::vector<uint8_t> out = me::amd::clahe(v, hdr[3], hdr[4], clip, &lut);
    std::FILE* fo = std::fopen(argv[2], "wb");
    if (!fo) {
      std::perror(argv[2]);
      return 2;
    }
    ok = std::fwrite(out.data(), 1, out.size(), fo) == out.size() &&
         std::fwrite(lut.data(), 1, lut.size(), fo) == lut.size();
    ok = (std::fclose(fo) == 0) && ok;
    if (!ok) {
      std::fprintf(stderr, "clahe_cli: write failed\n");
      return 2;
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "clahe_cli: %s\n", e.what());
    return 1;
  }
  return 0;
}
