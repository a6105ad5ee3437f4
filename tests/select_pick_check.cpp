// The shared steps of the radix select (visfd_amd/csrc/select_pick.hpp: select_pick_bin, select_rank) on hand-made
// histograms, checked against a sorted array: the bin that holds the k-th largest element and the rank left inside it.
// Plain host C++ -- the same function the host select, the slab select and the pick kernel run.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "select_pick.hpp"

static int g_bad = 0, g_checked = 0;

static void expect(bool ok, const char* what, long long a, long long b) {
  g_checked++;
  if (!ok) { g_bad++; std::printf("mismatch: %s (%lld, %lld)\n", what, a, b); }
}

// every k of a small histogram against the sorted multiset of bin numbers
static void against_sorted(const std::vector<uint64_t>& h, const char* what) {
  std::vector<int> keys;
  for (size_t b = 0; b < h.size(); b++)
    for (uint64_t c = 0; c < h[b]; c++) keys.push_back((int)b);
  std::sort(keys.begin(), keys.end(), [](int a, int b) { return a > b; });   // descending, as the reference sorts
  for (size_t k = 0; k < keys.size(); k++) {
    uint64_t r = k;
    const int bin = vh::select_pick_bin(h.data(), (int)h.size(), &r);
    expect(bin == keys[k], what, bin, keys[k]);
    // the rank inside the bin: elements of larger bins are gone
    const uint64_t above = (uint64_t)(std::find(keys.begin(), keys.end(), keys[k]) - keys.begin());
    expect(r == k - above, what, (long long)r, (long long)(k - above));
  }
  uint64_t r = keys.size();   // one past the end: no bin
  expect(vh::select_pick_bin(h.data(), (int)h.size(), &r) == -1, what, -1, -1);
  expect(r == keys.size(), "k untouched where no bin is found", (long long)r, (long long)keys.size());
  // the pick kernel's two levels (sums of 8 neighbouring bins, then the bins of one chunk) are the same walk
  if (h.size() % 8 == 0) {
    std::vector<uint64_t> chunk(h.size() / 8, 0);
    for (size_t b = 0; b < h.size(); b++) chunk[b / 8] += h[b];
    for (size_t k = 0; k < keys.size(); k++) {
      uint64_t r1 = k, r2 = k;
      const int flat = vh::select_pick_bin(h.data(), (int)h.size(), &r1);
      const int c = vh::select_pick_bin(chunk.data(), (int)chunk.size(), &r2);
      const int d = vh::select_pick_bin(h.data() + 8 * c, 8, &r2);
      expect(8 * c + d == flat && r1 == r2, "two-level walk", 8 * c + d, flat);
    }
  }
}

int main() {
  const int NB = 2048;
  {   // the cut in the top bin, in the bottom bin, all mass in one bin
    std::vector<uint64_t> h(NB, 0);
    h[NB - 1] = 5; h[1000] = 7; h[0] = 3;
    against_sorted(h, "top / middle / bottom bins");
    std::vector<uint64_t> one(NB, 0);
    one[777] = 40;
    against_sorted(one, "all mass in one bin");
    std::vector<uint64_t> bottom(NB, 0);
    bottom[0] = 9;
    against_sorted(bottom, "all mass in the bottom bin");
    std::vector<uint64_t> top(NB, 0);
    top[NB - 1] = 9;
    against_sorted(top, "all mass in the top bin");
  }
  {   // k on every bin boundary of a dense histogram (against_sorted walks every k), and a pseudo-random one
    std::vector<uint64_t> h(NB, 0);
    for (int b = 0; b < NB; b++) h[b] = (uint64_t)(b % 3);
    against_sorted(h, "dense histogram");
    uint32_t s = 12345u;
    for (int b = 0; b < NB; b++) { s = s * 1664525u + 1013904223u; h[b] = (s >> 24) % 5 == 0 ? (s >> 16) % 7 : 0; }
    against_sorted(h, "sparse pseudo-random histogram");
    std::vector<uint64_t> small(8, 0);
    small[7] = 2; small[3] = 1; small[0] = 4;
    against_sorted(small, "eight bins");
  }
  {   // 64-bit counts above 2^32: the running sum must not wrap at 32 bits
    std::vector<uint64_t> h(NB, 0);
    const uint64_t big = (1ull << 33) + 5;
    h[2000] = big; h[1500] = big; h[3] = 11;
    struct { uint64_t k; int bin; uint64_t rest; } cases[] = {
        {0, 2000, 0}, {big - 1, 2000, big - 1}, {big, 1500, 0}, {(1ull << 32) + 1, 2000, (1ull << 32) + 1},
        {2 * big - 1, 1500, big - 1}, {2 * big, 3, 0}, {2 * big + 10, 3, 10}};
    for (auto& c : cases) {
      uint64_t r = c.k;
      const int bin = vh::select_pick_bin(h.data(), NB, &r);
      expect(bin == c.bin && r == c.rest, "64-bit counts", bin, c.bin);
    }
    uint64_t r = 2 * big + 11;
    expect(vh::select_pick_bin(h.data(), NB, &r) == -1, "64-bit counts: past the end", 0, 0);
  }
  {   // the rank: floor of the SINGLE-precision product, and the reference's out-of-range read refused
    uint64_t k = 99;
    expect(vh::select_rank(1000, 0.05f, &k) && k == 50, "rank 1000 * 0.05", (long long)k, 50);
    expect(vh::select_rank(19, 0.05f, &k) && k == 0, "rank 19 * 0.05", (long long)k, 0);
    expect(!vh::select_rank(1000, 1.0f, &k), "fraction 1 selects no voxel", (long long)k, 1000);
    expect(!vh::select_rank(0, 0.5f, &k), "no voxel at all", 0, 0);
    expect(vh::select_rank(1000, 0.0f, &k) && k == 0, "fraction 0", (long long)k, 0);
    // 2^30 + 1 voxels: (float)n rounds to 2^30, so the product is exactly 2^29 and not 2^29 + 0.5
    expect(vh::select_rank((1ull << 30) + 1, 0.5f, &k) && k == (1ull << 29), "float conversion of n", (long long)k, 1ll << 29);
    const float f = std::nextafterf(1.0f, 0.0f);   // (float)(2^24 + 1) is 2^24, times 1 - 2^-24: exactly 2^24 - 1
    expect(vh::select_rank(16777217ull, f, &k) && k == 16777215ull, "rounded product", (long long)k, 16777215);
  }
  std::printf("checked %d facts, %d mismatches\n", g_checked, g_bad);
  return g_bad ? 1 : 0;
}
