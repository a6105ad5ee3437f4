// Compiled and run by tests/test_supervised.py: the reference-signature wrappers of the supervised blob thresholds in
// include/visfd_hip.hpp (FindSpheres, ChooseThreshold1D, FindBlobScores, ChooseBlobScoreThresholds[Multi],
// DiscardBlobsByScoreSupervised) under g++ -std=c++11 -Wall -Werror, on the host search (no GPU needed).
//   shim_supervised_check SCENE      SCENE: "n_blobs n_pos n_neg", then the blobs (x y z diameter score), the positive
//                                    and the negative training points (x y z), one per line
// stdout: one "name: values" line per result; then, after a line "progress:", what the wrappers reported.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>

#include "visfd_hip.hpp"

using namespace visfd;
typedef std::vector<std::array<float, 3> > Crds;

static Crds read_points(std::istream& in, size_t n) {
  Crds c(n);
  for (size_t i = 0; i < n; i++) in >> c[i][0] >> c[i][1] >> c[i][2];
  return c;
}

int main(int argc, char** argv) {
  if (argc != 2) return 64;
  std::ifstream in(argv[1]);
  size_t nb, np, nn;
  if (!(in >> nb >> np >> nn)) return 65;
  Crds bc(nb);
  std::vector<float> bd(nb), bs(nb);
  for (size_t i = 0; i < nb; i++) in >> bc[i][0] >> bc[i][1] >> bc[i][2] >> bd[i] >> bs[i];
  const Crds pos = read_points(in, np), neg = read_points(in, nn);
  if (!in) return 65;
  FindSpheresOnHost(true);
  std::cout.precision(9);
  std::ostringstream progress;

  std::vector<size_t> ids;
  FindSpheres(pos, ids, bc, bd, &progress);
  std::cout << "find_spheres:";
  for (size_t i = 0; i < ids.size(); i++) std::cout << " " << ids[i];
  std::cout << "\n";

  Crds kept_crds;
  std::vector<bool> accepted(np + nn, true), kept_accepted;
  for (size_t i = np; i < np + nn; i++) accepted[i] = false;
  Crds all(pos);
  all.insert(all.end(), neg.begin(), neg.end());
  std::vector<float> kept_scores;
  FindBlobScores(all, accepted, kept_crds, kept_accepted, kept_scores, bc, bd, bs, SORT_DECREASING_MAGNITUDE, &progress);
  std::cout << "blob_scores:";
  for (size_t i = 0; i < kept_scores.size(); i++) std::cout << " " << kept_scores[i] << (kept_accepted[i] ? "+" : "-");
  std::cout << "\n";
  if (kept_crds.size() != kept_scores.size() || kept_accepted.size() != kept_scores.size()) return 1;

  std::cout << "threshold_1d: " << ChooseThreshold1D(kept_scores, kept_accepted) << " "
            << ChooseThreshold1D(kept_scores, kept_accepted, false) << "\n";

  float lower = 0, upper = 0;
  ChooseBlobScoreThresholds(bc, bd, bs, pos, neg, &lower, &upper, SORT_DECREASING_MAGNITUDE, &progress);
  std::cout << "thresholds: " << lower << " " << upper << "\n";

  // two sets: the list and its first half, each with all the training points
  std::vector<Crds> mc(2, bc), mp(2, pos), mn(2, neg);
  std::vector<std::vector<float> > md(2, bd), ms(2, bs);
  mc[1].resize(nb / 2); md[1].resize(nb / 2); ms[1].resize(nb / 2);
  float mlower = 0, mupper = 0;
  ChooseBlobScoreThresholdsMulti(mc, md, ms, mp, mn, &mlower, &mupper, SORT_DECREASING_MAGNITUDE, &progress);
  std::cout << "thresholds_multi: " << mlower << " " << mupper << "\n";

  float dlower = 0, dupper = 0;
  DiscardBlobsByScoreSupervised(bc, bd, bs, pos, neg, SORT_DECREASING_MAGNITUDE, &dlower, &dupper, &progress);
  if (dlower != lower || dupper != upper) return 2;
  std::cout << "kept:";
  for (size_t i = 0; i < bc.size(); i++) std::cout << " " << bc[i][0] << "," << bc[i][1] << "," << bc[i][2] << "," << bd[i] << "," << bs[i];
  std::cout << "\n";

  // an empty negative set: the reference's exception, its text verbatim
  try {
    ChooseBlobScoreThresholds(bc, bd, bs, pos, Crds(), &lower, &upper);
    return 3;
  } catch (VisfdErr& e) {
    if (std::string(e.what()).find("Error: Empty list of negative training examples.\n") != 0) return 4;
  }
  std::cout << "progress:\n" << progress.str();
  return 0;
}
