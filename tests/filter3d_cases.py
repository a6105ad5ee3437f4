"""The filter_mrc command lines behind tests/golden/filter3d.npz, shared by the generator (golden/make_golden_filter3d.py)
and the tests.  Inputs are rebuilt from seeds (volgen); the file holds the reference program's outputs only."""
import volgen

# name -> (shape (nz, ny, nx), masked, filter_mrc arguments, what the arguments mean to the restatement, seed)
# The seed is written out per case: the committed outputs belong to it, whatever cases come and go around it.
# kind "ggauss": width (x, y, z), m, ratio (< 0: from the 0.03 threshold), normalize
# kind "dogg":   width_a, width_b, m, n, ratio
# kind "fluct":  radius, exponent, ratio, normalize
CASES = {
    "ggauss_m3": ((16, 20, 24), False, ["-ggauss", "1.6", "-exponent", "3"],
                  ("ggauss", (1.6, 1.6, 1.6), 3.0, -1.0, True), 906),
    "ggauss_m3_mask": ((16, 20, 24), True, ["-ggauss", "1.6", "-gauss-exponent", "3"],
                       ("ggauss", (1.6, 1.6, 1.6), 3.0, -1.0, True), 907),
    # half-widths floor(2 * (2.2, 1.1, 0.6)) = (4, 2, 1)
    "ggauss_aniso": ((14, 18, 30), False, ["-ggauss-aniso", "2.2", "1.1", "0.6", "-exponent", "1.5", "-truncate", "2"],
                     ("ggauss", (2.2, 1.1, 0.6), 1.5, 2.0, True), 905),
    "ggauss_nonorm": ((16, 20, 24), False, ["-ggauss", "1.6", "-exponent", "3", "-normalize-filters", "no"],
                      ("ggauss", (1.6, 1.6, 1.6), 3.0, -1.0, False), 908),
    "dogg": ((16, 20, 24), False, ["-dogg", "1.2", "2.0", "-exponents", "2", "4", "-truncate", "2.5"],
             ("dogg", (1.2, 1.2, 1.2), (2.0, 2.0, 2.0), 2.0, 4.0, 2.5), 900),
    # the two windows from the 0.03 threshold, each with its own exponent
    "dogg_threshold": ((16, 20, 24), False, ["-dogg", "1.2", "2.0", "-gdog-exponents", "2", "4"],
                       ("dogg", (1.2, 1.2, 1.2), (2.0, 2.0, 2.0), 2.0, 4.0, -1.0), 902),
    "dogg_aniso": ((14, 18, 30), False,
                   ["-dogg-aniso", "1.0", "1.5", "0.8", "2.0", "1.2", "1.6", "-exponents", "3", "1.5", "-truncate", "2"],
                   ("dogg", (1.0, 1.5, 0.8), (2.0, 1.2, 1.6), 3.0, 1.5, 2.0), 901),
    "fluct_m6": ((16, 20, 24), False, ["-fluct", "3", "-exponent", "6"], ("fluct", (3.0, 3.0, 3.0), 6.0, -1.0, True), 903),
    "fluct_m6_mask": ((16, 20, 24), True, ["-fluct", "3", "-exponent", "6"], ("fluct", (3.0, 3.0, 3.0), 6.0, -1.0, True), 904),
    # half-width 6 in z, 5 planes
    "ggauss_wide_z": ((5, 20, 24), False, ["-ggauss", "3", "-exponent", "4", "-truncate", "2"],
                      ("ggauss", (3.0, 3.0, 3.0), 4.0, 2.0, True), 909),
}
# Not recorded: "-dogg ... -mask".  The reference program applies the filter with a mask and without a denominator and
# dereferences a null pointer at the first masked voxel (filter3d.hpp:182): it does not exit 0.


def inputs(name):
    shape, masked, seed = CASES[name][0], CASES[name][1], CASES[name][4]
    src = volgen.noise_volume(shape, seed=seed)
    mask = volgen.block_mask(shape, seed=seed + 50) if masked else None
    return src, mask
