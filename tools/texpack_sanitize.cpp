// tools/texpack_sanitize.cpp - the texture packer's host side (fspt_amd/csrc/fspt_texpack_check.hpp: the argument checks and the
// per-layer records) as a stand-alone program for AddressSanitizer + UndefinedBehaviorSanitizer on the CPU
// (tools/texpack_sanitize.sh).  Every refusal of the checks, patches included, and the records of descriptions with unused,
// shared and no images; exits 0 when every answer is the expected one.
#include "../fspt_amd/csrc/fspt_texpack_check.hpp"

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <limits>
#include <memory>

static char g_err[512];
void fspt_set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
}

namespace {
int g_failed = 0;
void expect(bool ok, const char *what) {
  if (!ok) { std::printf("FAILED: %s (last error: %s)\n", what, g_err); ++g_failed; }
}

// a description that owns exactly the bytes it declares: a read past an image or a list is the sanitizer's to find
struct Desc {
  std::vector<std::unique_ptr<uint8_t[]>> px;
  std::vector<fspt_texture_image> images;
  std::vector<fspt_texture_layer> layers;
  fspt_texture_pack p{};
  void image(uint32_t w, uint32_t h) {
    px.emplace_back(new uint8_t[(size_t)w * h * 4]());
    images.push_back({px.back().get(), w, h});
  }
  void layer(int32_t kind, uint32_t image = 0, uint32_t corrected = 0, std::array<uint8_t, 4> sw = {0, 1, 2, 3}, std::array<float, 3> c = {0.1f, 0.2f, 0.3f}) {
    fspt_texture_layer y{};
    y.kind = kind; y.image = image; y.corrected = corrected;
    for (int k = 0; k < 4; ++k) y.swizzle[k] = sw[k];
    for (int k = 0; k < 3; ++k) y.color[k] = c[k];
    layers.push_back(y);
  }
  const fspt_texture_pack *pack(uint32_t res) {
    p.images = images.data(); p.n_images = (uint32_t)images.size(); p.layers = layers.data(); p.n_layers = (uint32_t)layers.size(); p.res = res;
    return &p;
  }
};

Desc good(uint32_t res = 4) {
  Desc d;
  d.image(3, 5); d.image(res, res); d.image(7, 2); // (the last one is used by no layer)
  d.layer(FSPT_TEXLAYER_COLOR);
  d.layer(FSPT_TEXLAYER_IMAGE, 0, 1, {0, 2, 1, 3});
  d.layer(FSPT_TEXLAYER_PIXELS, 1);
  d.layer(FSPT_TEXLAYER_IMAGE, 0, 0, {1, 1, 1, 1});
  return d;
}
} // namespace

int main() {
  using namespace fspt;
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  { Desc d = good(); expect(texpack_check("t", d.pack(4), false) == FSPT_OK, "a good description"); }
  const std::pair<const char *, std::function<void(Desc &)>> spoil[] = {
      {"res 0", [](Desc &d) { d.p.res = 0; }}, {"res 16385", [](Desc &d) { d.p.res = 16385; }}, {"no layers", [](Desc &d) { d.p.n_layers = 0; }},
      {"NULL layers", [](Desc &d) { d.p.layers = nullptr; }}, {"NULL images", [](Desc &d) { d.p.images = nullptr; }},
      {"NULL rgba", [](Desc &d) { d.images[2].rgba = nullptr; }}, {"w 0", [](Desc &d) { d.images[0].w = 0; }}, {"h 16385", [](Desc &d) { d.images[0].h = 16385; }},
      {"image index", [](Desc &d) { d.layers[1].image = 3; }}, {"image index 2^32 - 1", [](Desc &d) { d.layers[2].image = 0xFFFFFFFFu; }},
      {"swizzle 4", [](Desc &d) { d.layers[3].swizzle[3] = 4; }}, {"swizzle 255", [](Desc &d) { d.layers[1].swizzle[0] = 255; }},
      {"kind 3", [](Desc &d) { d.layers[0].kind = 3; }}, {"kind INT32_MIN", [](Desc &d) { d.layers[0].kind = INT32_MIN; }},
      {"colour NaN", [nan](Desc &d) { d.layers[0].color[2] = nan; }}, {"colour -inf", [inf](Desc &d) { d.layers[0].color[0] = -inf; }},
      {"pixels not res x res", [](Desc &d) { d.layers[2].image = 0; }}};
  for (const auto &s : spoil) {
    Desc d = good();
    d.pack(4);
    s.second(d);
    expect(texpack_check("t", &d.p, false) == FSPT_E_INVALID, s.first);
    const uint32_t ids[4] = {0, 1, 2, 3};
    expect(texpack_check("t", &d.p, false, ids, d.p.n_layers, 8, 4, true) == FSPT_E_INVALID, s.first);
  }
  expect(texpack_check("t", nullptr, false) == FSPT_E_INVALID, "NULL description");
  { // the device form looks at the alignment only
    Desc d = good(); d.pack(4);
    expect(texpack_check("t", &d.p, true) == FSPT_OK, "aligned device sources");
    d.images[2].rgba += 2;
    expect(texpack_check("t", &d.p, true) == FSPT_E_INVALID, "a misaligned device source");
    expect(texpack_check("t", &d.p, false) == FSPT_OK, "... which a host source may be");
  }
  { // patches
    Desc d = good(); d.pack(4);
    const uint32_t ids[4] = {5, 0, 7, 2}, twice[4] = {5, 0, 5, 2}, high[4] = {5, 0, 8, 2};
    expect(texpack_check("t", &d.p, false, ids, 4, 8, 4, true) == FSPT_OK, "a good patch");
    expect(texpack_check("t", &d.p, false, nullptr, 4, 8, 4, true) == FSPT_E_INVALID, "NULL layer ids");
    expect(texpack_check("t", &d.p, false, ids, 3, 8, 4, true) == FSPT_E_INVALID, "fewer ids than layers");
    expect(texpack_check("t", &d.p, false, twice, 4, 8, 4, true) == FSPT_E_INVALID, "a layer id twice");
    expect(texpack_check("t", &d.p, false, high, 4, 8, 4, true) == FSPT_E_INVALID, "a layer id at raw_layers");
    expect(texpack_check("t", &d.p, false, ids, 4, 8, 9, true) == FSPT_E_INVALID, "another res than the retained atlas's");
    expect(texpack_check("t", &d.p, false, ids, 4, 0, 0, true) == FSPT_OK, "no retained atlas: the caller's FSPT_E_STATE");
    std::vector<TexLayerRec> rec; std::vector<uint64_t> off; uint64_t bytes = 0;
    texpack_records(&d.p, false, ids, rec, off, &bytes);
    expect(rec.size() == 4 && rec[0].dst == 5 && rec[2].dst == 7 && rec[3].dst == 2, "a patch's records write its layers");
  }
  { // records: an image two layers use is uploaded once, an unused one not at all; flags and colours
    Desc d = good(); d.pack(4);
    std::vector<TexLayerRec> rec; std::vector<uint64_t> off; uint64_t bytes = 0;
    texpack_records(&d.p, false, nullptr, rec, off, &bytes);
    expect(bytes == 3 * 5 * 4 + 4 * 4 * 4 && off[0] == 0 && off[1] == 60 && off[2] == UINT64_MAX, "the upload holds the used images once");
    expect(rec[1].src == 0 && rec[3].src == 0 && rec[2].src == 60 && rec[1].w == 3 && rec[1].h == 5, "the records' sources");
    expect(rec[1].flags == (1u | 4u | (0u << 8) | (2u << 10) | (1u << 12) | (3u << 14)) && rec[3].flags == (1u | (1u << 8) | (1u << 10) | (1u << 12) | (1u << 14)) &&
               rec[2].flags == 2u && rec[0].flags == 0u, "the records' flags");
    const float c[3] = {0.1f, 0.2f, 0.3f}, edge[3] = {-1.0f, 2.0f, 0.5f / 255.0f};
    expect(rec[0].color == tex_color_texel(c) && tex_color_texel(c) == (0xFF000000u | 26u | (51u << 8) | (77u << 16)), "a colour's texel");  // 0.3f * 255 + 0.5 = 77.0000003
    expect(tex_color_texel(edge) == (0xFF000000u | 0u | (255u << 8) | (1u << 16)), "a colour clamps and rounds half up");
    texpack_records(&d.p, true, nullptr, rec, off, &bytes);
    expect(rec[1].src == (uint64_t)(uintptr_t)d.images[0].rgba && rec[2].src == (uint64_t)(uintptr_t)d.images[1].rgba, "the device form's records point at the sources");
  }
  { // colours only: no image list at all
    Desc d; d.layer(FSPT_TEXLAYER_COLOR);
    expect(texpack_check("t", d.pack(1), false) == FSPT_OK, "a colours-only description");
    std::vector<TexLayerRec> rec; std::vector<uint64_t> off; uint64_t bytes = 1;
    texpack_records(&d.p, false, nullptr, rec, off, &bytes);
    expect(bytes == 0 && off.empty() && rec.size() == 1, "... uploads nothing");
  }
  std::printf(g_failed ? "%d checks failed\n" : "texpack host checks: all passed\n", g_failed);
  return g_failed ? 1 : 0;
}
