// orb_detect -- chip_orb_detect against a plain C++ restatement of its definition (include/cerebro_hip.h, "ORB keypoint detection on the
// device"), record for record, on a synthetic textured 752 x 480 frame at the defaults and on a grid of identical dots (equal Harris
// keys: the selection is decided by the raster index alone).  Exits 0 when both agree.
//   orb_detect            compare
//   orb_detect REPS       compare, then time both: the device call (median of REPS) and the host restatement (a plain loop, not OpenCV's
//                         implementation)
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "cerebro_hip.h"

namespace {

using Image = std::vector<uint8_t>;
const int kRing[16][2] = {{0, -3}, {1, -3}, {2, -2}, {3, -1}, {3, 0}, {3, 1}, {2, 2}, {1, 3}, {0, 3}, {-1, 3}, {-2, 2}, {-3, 1}, {-3, 0}, {-3, -1}, {-2, -2}, {-1, -3}};
const int kUmax[16] = {15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3};

void axis(int i, int n_src, int n_dst, int *i0, int *i1, int64_t *frac)
{
    int64_t X = ((int64_t)(2 * i + 1) * n_src * 1024) / n_dst - 1024;
    X = std::min(std::max<int64_t>(X, 0), (int64_t)(n_src - 1) * 2048);
    *i0 = (int)(X >> 11); *frac = X & 2047; *i1 = std::min(*i0 + 1, n_src - 1);
}

Image downsample(const Image &src, int ws, int hs, int w, int h)
{
    Image out((size_t)w * h);
    for (int y = 0; y < h; y++) {
        int y0, y1; int64_t b;
        axis(y, hs, h, &y0, &y1, &b);
        for (int x = 0; x < w; x++) {
            int x0, x1; int64_t a;
            axis(x, ws, w, &x0, &x1, &a);
            const int64_t v = src[(size_t)y0 * ws + x0] * (2048 - a) * (2048 - b) + src[(size_t)y0 * ws + x1] * a * (2048 - b) +
                              src[(size_t)y1 * ws + x0] * (2048 - a) * b + src[(size_t)y1 * ws + x1] * a * b + (1 << 21);
            out[(size_t)y * w + x] = (uint8_t)(v >> 22);
        }
    }
    return out;
}

int fast_score(const Image &im, int w, int x, int y)
{
    const int ip = im[(size_t)y * w + x];
    int d[16];
    for (int k = 0; k < 16; k++) d[k] = im[(size_t)(y + kRing[k][1]) * w + x + kRing[k][0]] - ip;
    int b = -256, dd = -256;
    for (int k = 0; k < 16; k++) {
        int lo = 256, hi = 256;
        for (int j = 0; j < 9; j++) { lo = std::min(lo, d[(k + j) & 15]); hi = std::min(hi, -d[(k + j) & 15]); }
        b = std::max(b, lo); dd = std::max(dd, hi);
    }
    return std::max(b, dd) - 1;
}

int64_t harris(const Image &im, int w, int x, int y)
{
    int64_t a = 0, bb = 0, c = 0;
    for (int dy = -3; dy <= 3; dy++)
        for (int dx = -3; dx <= 3; dx++) {
            const auto p = [&](int j, int i) { return (int)im[(size_t)(y + dy + j) * w + x + dx + i]; };
            const int ix = 2 * (p(0, 1) - p(0, -1)) + (p(-1, 1) - p(-1, -1)) + (p(1, 1) - p(1, -1));
            const int iy = 2 * (p(1, 0) - p(-1, 0)) + (p(1, -1) - p(-1, -1)) + (p(1, 1) - p(-1, 1));
            a += ix * ix; bb += iy * iy; c += ix * iy;
        }
    return 25 * (a * bb - c * c) - (a + bb) * (a + bb);
}

// the definition, level by level
std::vector<chip_orb_keypoint> restate(const Image &image, int width, int height, const chip_orb_params &p, int32_t counts[8])
{
    chip_orb_level lv[8];
    if (chip_orb_plan(width, height, &p, lv) != CHIP_OK) std::exit(2);
    std::vector<chip_orb_keypoint> out;
    Image im = image;
    for (int l = 0; l < 8; l++) counts[l] = 0;
    for (int l = 0; l < p.n_levels; l++) {
        const int w = lv[l].width, h = lv[l].height;
        if (w < 1 || h < 1) break;
        if (l > 0) im = downsample(im, lv[l - 1].width, lv[l - 1].height, w, h);
        if (lv[l].x1 < lv[l].x0) continue;
        std::vector<int16_t> S((size_t)w * h, -256);
        for (int y = 3; y < h - 3; y++)
            for (int x = 3; x < w - 3; x++) S[(size_t)y * w + x] = (int16_t)fast_score(im, w, x, y);
        struct Cand { int64_t R; int raster; };
        std::vector<Cand> cand;
        for (int y = lv[l].y0; y <= lv[l].y1; y++)
            for (int x = lv[l].x0; x <= lv[l].x1; x++) {
                const int s = S[(size_t)y * w + x];
                bool ok = s >= p.fast_threshold;
                for (int dy = -1; dy <= 1 && ok; dy++)
                    for (int dx = -1; dx <= 1; dx++)
                        if ((dx || dy) && s <= S[(size_t)(y + dy) * w + x + dx]) ok = false;
                if (ok) cand.push_back(Cand{harris(im, w, x, y), y * w + x});
            }
        if ((int)cand.size() > lv[l].quota) {
            std::sort(cand.begin(), cand.end(), [](const Cand &a, const Cand &b) { return a.R != b.R ? a.R > b.R : a.raster < b.raster; });
            cand.resize((size_t)lv[l].quota);
            std::sort(cand.begin(), cand.end(), [](const Cand &a, const Cand &b) { return a.raster < b.raster; });
        }
        for (const Cand &c : cand) {
            const int y = c.raster / w, x = c.raster % w;
            chip_orb_keypoint k{};
            k.response = c.R;
            k.x = (float)((double)x * lv[l].scale); k.y = (float)((double)y * lv[l].scale);
            for (int v = -15; v <= 15; v++)
                for (int u = -kUmax[std::abs(v)]; u <= kUmax[std::abs(v)]; u++) {
                    const int I = im[(size_t)(y + v) * w + x + u];
                    k.m10 += u * I; k.m01 += v * I;
                }
            k.x_level = (uint16_t)x; k.y_level = (uint16_t)y; k.level = (uint16_t)l;
            out.push_back(k);
        }
        counts[l] = (int32_t)cand.size();
    }
    return out;
}

Image textured(int w, int h, unsigned seed)
{
    std::mt19937 rng(seed);
    const int cell = 5, bw = (w + cell - 1) / cell;
    std::vector<int> blocks((size_t)bw * ((h + cell - 1) / cell));
    for (int &b : blocks) b = 30 + (int)(rng() % 196);
    Image im((size_t)w * h);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) im[(size_t)y * w + x] = (uint8_t)std::min(255, std::max(0, blocks[(size_t)(y / cell) * bw + x / cell] + (int)(rng() % 51) - 25));
    return im;
}

double ms_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

bool compare(chip_ctx *chip, const char *what, const Image &im, int w, int h, const chip_orb_params &p, int reps)
{
    std::vector<chip_orb_keypoint> got((size_t)p.n_features);
    int32_t n = -1, counts[8], want_counts[8];
    const int rc = chip_orb_detect(chip, im.data(), w, h, &p, got.data(), p.n_features, &n, counts);
    if (rc != CHIP_OK) { std::fprintf(stderr, "chip_orb_detect -> %s\n", chip_strerror(rc)); return false; }
    auto t0 = std::chrono::steady_clock::now();
    const std::vector<chip_orb_keypoint> want = restate(im, w, h, p, want_counts);
    const double host_ms = ms_since(t0);
    const bool same = n == (int32_t)want.size() && !std::memcmp(counts, want_counts, sizeof counts) &&
                      (n == 0 || !std::memcmp(got.data(), want.data(), (size_t)n * sizeof(chip_orb_keypoint)));
    std::printf("%-22s %4d x %-4d n = %5d  levels %d %d %d %d %d %d %d %d  %s the host restatement\n", what, w, h, n, counts[0], counts[1], counts[2],
                counts[3], counts[4], counts[5], counts[6], counts[7], same ? "==" : "DIFFERS from");
    if (same && reps > 0) {
        std::vector<double> t;
        for (int r = 0; r < reps; r++) {
            t0 = std::chrono::steady_clock::now();
            if (chip_orb_detect(chip, im.data(), w, h, &p, got.data(), p.n_features, &n, nullptr) != CHIP_OK) return false;
            t.push_back(ms_since(t0));
        }
        std::sort(t.begin(), t.end());
        std::printf("    chip_orb_detect %.3f ms (median of %d); the host restatement %.1f ms (a plain loop, not OpenCV's implementation)\n",
                    t[t.size() / 2], reps, host_ms);
    }
    return same;
}

}  // namespace

int main(int argc, char **argv)
{
    const int reps = argc > 1 ? std::atoi(argv[1]) : 0;
    chip_ctx *chip = nullptr;
    int rc = chip_create(&chip, 4096, 0, 0, 0, 1);
    if (rc != CHIP_OK) { std::fprintf(stderr, "chip_create -> %s\n", chip_strerror(rc)); return 2; }
    chip_orb_params p;
    chip_orb_params_default(&p);
    bool ok = compare(chip, "textured frame", textured(752, 480, 752480u), 752, 480, p, reps);
    // 40 x 30 identical isolated dots, 8 apart, one level, room for 1000 of the 1200: the first 1000 in raster order
    const int w = 2 * 31 + 39 * 8 + 1, h = 2 * 31 + 29 * 8 + 1;
    Image dots((size_t)w * h, 50);
    for (int j = 0; j < 30; j++)
        for (int i = 0; i < 40; i++) dots[(size_t)(31 + 8 * j) * w + 31 + 8 * i] = 200;
    chip_orb_params q = p;
    q.n_levels = 1; q.n_features = 1000;
    ok = compare(chip, "dot pattern", dots, w, h, q, reps) && ok;
    chip_destroy(chip);
    return ok ? 0 : 1;
}
