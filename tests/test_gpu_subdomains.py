"""Subdomain sweep: decomposed parity at every rank size that switches a path.

The depth sweep (tests/test_gpu_depths.py) and the width sweep
(tests/test_gpu_widths.py) pin every column and tile / strip / block switch
to the oracle on a single domain, which has walls (or periodic images) on all
four sides at once.  A rank of a decomposed run has its own Lm, Mm and its own
subset of walls, and the same host predicates then pick paths that no
single-domain size reaches:
  * k_step2d.hip launch_step2d widens a rank's fast step by ext = 2 (gend -
    iif) cells (6, 4, 2, 0 at the default interval K = 4) on every rank
    boundary, and launch_fast_step takes s2d_edge_mode on the widened bounds.
    A rank with the east wall and none to the west starts its tiles at
    tile_i0(1 - ext) = -15 for ext > 0 and 1 for ext = 0, so a rank 48
    columns wide takes the separate edge launches while ext > 0 and folds at
    ext = 0, a rank 64 wide the opposite; a rank with the north wall and none
    to the south folds unless (Mm + ext) % 4 == 0.  Model.horizontal_path()
    names the mode of the rank's own bounds; Model.fast_step_edge_modes() the
    modes the fast steps of the last enqueued step took;
  * k_prsgrd_strip.hip: xedge, xlo / xhi and own on a rank with the east wall
    only (strip 0 no edge strip, the last one is), the west wall only, or no
    wall in a closed basin; prsgrd_strip_rows gives jA = 1 on a rank with no
    south wall and jB = Mm with no north wall, so the row chunks
    (ROMS_PRS_STRIP_J = 8) fill at other heights than on a single domain;
  * a rank of a closed basin that touches no wall (the centre of 3 x 3): edge
    mode 0 without periodic images, no edge strip, all four corner exchanges;
  * rank widths on a 16-column block boundary (seg_grid_of, chain_grid_of),
    on the 31 / 32 omega_takes_seg switch and on the 60 / 61 strip boundary;
  * the smallest ranks roms_gpu_init accepts (Lm, Mm >= 2), whose 2-deep
    halo is the neighbour's whole interior; the fast-loop interval falls to 1.
ENTRIES names, per entry, the family, the global grid, the processor grid,
the exchange interval asked for and taken, and for each rank its extents
(re-derived from romsgpu.rank_extent), horizontal_path(), the edge-mode set
and one phrase on what the entry is there for.  Every rank asserts these in
run_decomposed's probe after the steps, so an entry that silently stops
exercising its switch fails.  The mode sets are those s2d_edge_mode gives for
ext in {0, 2, .., 2 (K - 1)}: predicted() below is the predicate written out
in Python, and test_table_matches_predicates holds the table to it.

Families (cells as in the width sweep: basin 2 km, Filament 200 m x 50 m):
"kpp" the closed split-EOS basin with KPP and surface fluxes at N = 12,
"n100" the same at N = 100 (segment solvers, v-tiles), "fold" the closed
basin without LMD at N = 12, "filament" the doubly periodic Filament at
N = 10, "open" the basin with four open edges, the island and LMD, no sponge
(tests/test_gpu_multirank.py basin_obc), at N = 10.

Per entry: (a) check_decomposition -- owned cells, and the halos of the
exchanged fields, equal the single-domain window bitwise, no tolerance;
(c) the per-rank paths.  Per distinct global grid and family: (b) the single
domain, 12 steps, against the CPU oracle within RMS_RUN, so the bitwise chain
ends at the high-precision reference.  test_subdomain_variants_bitwise tells
which form is wrong when (a) fails at a strip entry.

What the sweep found: six entries failed (a) as the library stood, with NaN
after one step on every rank -- strip-kpp-121x18-2x2, strip-kpp-121x20-2x2,
strip-fil-121-2x1, strip-fil-121x18-2x2 and both nowall-54x42-3x3 entries --
at every K and with strips or tiles alike.  halo.hip sized the message slots
of the send and receive buffers from the rank's own largest message, while a
neighbour's buffers are addressed with the reader's (in-process copies) or
the writer's (IPC peer writes) slot size; the sizes differ when the ranks'
extents do (121 = 61 + 60 with north / south messages) or their neighbours
do (the 3 x 3 centre beside ranks with a wall).  halo_setup now takes the
largest of any rank.  No predicate was wrong, and the smallest ranks (4, 3
and 2 columns or rows, closed and periodic) reproduce the single domain, so
roms_gpu_init refuses no split it accepted.

What the sweep catches, tried in a scratch copy of the kernels (predicates
only, nothing of it committed), every test of this file:
  * launch_fast_step taking its mode from the un-widened bounds fails the
    path assertion of every entry whose table names {1, 2} and no other (11
    entries; fold-26-1x2 and fold-96-2x1-K1 pass).  In the numbers it fails
    where the base mode folds and a widened step must not: fold-96-2x1 and
    its K = 2, 3 forms on the east rank (v 2e-4, u 7e-10), fold-96x28-2x2
    (1e-12), strip-kpp-121x20-2x2 and 240x20 (2e-11), fold-28-1x2 and both
    3 x 3 entries (1e-14 .. 1e-18); fold-128-2x1 and fold-24-1x2 stay bitwise,
    their base mode being the edge launches, which are right at every ext.
    The decompositions of tests/test_gpu_multirank.py catch it too (zeta
    1.5e-9): their 36 x 28 basin split in y has north ranks with Mm = 14.
  * `xedge` as `c0 + 61 > G.xhi` fails (a) on the east rank (Lm = 60, one
    full strip that is the east edge strip only) of strip-kpp-121-2x1,
    strip-kpp-121x18-2x2, strip-kpp-121x20-2x2 (zeta 2.5e-9, u 2.6e-8) and
    open-121-2x1 (zeta 3.5e-6), and the prs_tiles variant at both sizes.
    The 120-wide east ranks of the 240 entries stay bitwise equal to the
    single domain, which takes the same wrong strip at the same columns (240
    = 4 full strips): there (b) fails, kpp 240x5, 240x18, 240x20 and 180x5
    (field RMS 1e-9 .. 8e-9 against RMS_RUN 1e-10).  Every other test passes.
  * prsgrd_strip_rows with jA = 3 on a rank with no south wall fails the path
    assertion of every rank whose table names jA = 1 (22 entries, the north
    ranks of the 2 x 2 strip entries among them) and nothing in the numbers:
    launch_prsgrd hands the rows below jA to the tiles, which are bitwise the
    strips, so this error costs speed and not correctness.
Measured errors and the table: DESIGN.md section 4.
"""
import numpy as np
import pytest

import oracle
import romsgpu
from test_gpu_multirank import check_decomposition, run_decomposed
from test_gpu_parity import PROGNOSTIC, RMS_RUN, basin_cfg, check_fields
from test_gpu_widths import BITWISE_FIELDS, environ

pytestmark = pytest.mark.gpu

FAMILY_N = {"kpp": 12, "n100": 100, "fold": 12, "filament": 10, "open": 10}

# name -> (family, LLm, MMm, np_xi, np_eta, ROMS_GPU_S2D_K asked for (None: the default 4), interval K taken,
#          whole steps, per rank in rank order (inode fastest) (Lm, Mm, closed-edge mode of the rank's own bounds,
#          prsgrd strips (per row, jA, jB) or None, omega in the segment form, edge modes of the fast steps),
#          what the entry is there for)
ENTRIES = {
    # ---- prsgrd strips, closed KPP basin split in x.  MMm = 5: the smallest height whose 2-way y split
    # ([3, 2]) leaves the south rank (rows 3..Mm_r) a strip row; K = 1 as 2K + 2 must fit 5 rows
    "strip-kpp-121-2x1": ("kpp", 121, 5, 2, 1, None, 1, 4, [
        (61, 5, 2, (2, 3, 4), True, {2}),
        (60, 5, 2, (1, 3, 4), True, {2}),
    ], "west rank: a second strip of one column that is no edge strip; east rank: one full strip, east edge only"),
    "strip-kpp-240-2x1": ("kpp", 240, 5, 2, 1, None, 1, 4, [
        (120, 5, 2, (2, 3, 4), True, {2}),
        (120, 5, 2, (2, 3, 4), True, {2}),
    ], "east rank: two full strips, iend + 1 on lane 62 of the last with no west wall on the first"),
    "strip-kpp-180-3x1": ("kpp", 180, 5, 3, 1, None, 1, 4, [
        (60, 5, 2, (1, 3, 4), True, {2}),
        (60, 5, 2, (1, 3, 4), True, {2}),
        (60, 5, 2, (1, 3, 4), True, {2}),
    ], "middle rank: one full strip with xedge false in a closed basin"),
    "strip-kpp-183-3x1": ("kpp", 183, 5, 3, 1, None, 1, 4, [
        (61, 5, 2, (2, 3, 4), True, {2}),
        (61, 5, 2, (2, 3, 4), True, {2}),
        (61, 5, 2, (2, 3, 4), True, {2}),
    ], "middle rank: a second strip of one column, no edge strip at all"),
    # ---- the same widths 2 x 2: the north ranks' strip rows 1..Mm_r - 1 are one full chunk of 8 at
    # Mm_r = 9 and spill one row into a second chunk at Mm_r = 10
    "strip-kpp-121x18-2x2": ("kpp", 121, 18, 2, 2, None, 3, 4, [
        (61, 9, 2, (2, 3, 9), True, {2}),
        (60, 9, 2, (1, 3, 9), True, {2}),
        (61, 9, 2, (2, 1, 8), True, {2}),
        (60, 9, 2, (1, 1, 8), True, {2}),
    ], "north ranks: rows 1..8, exactly one row chunk; south ranks: rows 3..9"),
    "strip-kpp-121x20-2x2": ("kpp", 121, 20, 2, 2, None, 4, 4, [
        (61, 10, 2, (2, 3, 10), True, {2}),
        (60, 10, 2, (1, 3, 10), True, {2}),
        (61, 10, 2, (2, 1, 9), True, {1, 2}),
        (60, 10, 2, (1, 1, 9), True, {1, 2}),
    ], "north ranks: rows 1..9, a second chunk of one row; (10 + ext) % 4 == 0 at ext 2 and 6"),
    "strip-kpp-240x18-2x2": ("kpp", 240, 18, 2, 2, None, 3, 4, [
        (120, 9, 2, (2, 3, 9), True, {2}),
        (120, 9, 2, (2, 3, 9), True, {2}),
        (120, 9, 2, (2, 1, 8), True, {2}),
        (120, 9, 2, (2, 1, 8), True, {2}),
    ], "120-wide east ranks with the north or the south wall; north ranks one full row chunk"),
    "strip-kpp-240x20-2x2": ("kpp", 240, 20, 2, 2, None, 4, 4, [
        (120, 10, 2, (2, 3, 10), True, {2}),
        (120, 10, 2, (2, 3, 10), True, {2}),
        (120, 10, 2, (2, 1, 9), True, {1, 2}),
        (120, 10, 2, (2, 1, 9), True, {1, 2}),
    ], "120-wide east ranks; north ranks a second chunk of one row"),
    # ---- strips, Filament: every exchange is a rank boundary and none is a wall
    "strip-fil-121-2x1": ("filament", 121, 9, 2, 1, None, 3, 4, [
        (61, 9, 0, (2, 1, 9), True, {0}),
        (60, 9, 0, (1, 1, 9), True, {0}),
    ], "periodic: a second strip of one column beside a rank boundary; one full strip fed from both neighbours"),
    "strip-fil-180-3x1": ("filament", 180, 9, 3, 1, None, 3, 4, [
        (60, 9, 0, (1, 1, 9), True, {0}),
        (60, 9, 0, (1, 1, 9), True, {0}),
        (60, 9, 0, (1, 1, 9), True, {0}),
    ], "periodic: three full strips, each a rank"),
    "strip-fil-121x18-2x2": ("filament", 121, 18, 2, 2, None, 3, 4, [
        (61, 9, 0, (2, 1, 9), True, {0}),
        (60, 9, 0, (1, 1, 9), True, {0}),
        (61, 9, 0, (2, 1, 9), True, {0}),
        (60, 9, 0, (1, 1, 9), True, {0}),
    ], "periodic 2 x 2: strip rows 1..9 on every rank, corner exchanges through the periodic seam"),
    # ---- the fold decided per fast step, basin without LMD
    "fold-96-2x1": ("fold", 96, 10, 2, 1, None, 4, 4, [
        (48, 10, 2, (1, 3, 9), True, {2}),
        (48, 10, 2, (1, 3, 9), True, {1, 2}),
    ], "east rank 48 wide: edge launches at ext 6, 4, 2 ((48 + 16) % 64 == 0), folded at ext 0"),
    "fold-128-2x1": ("fold", 128, 10, 2, 1, None, 4, 4, [
        (64, 10, 2, (2, 3, 9), True, {2}),
        (64, 10, 1, (2, 3, 9), True, {1, 2}),
    ], "east rank 64 wide: folded at ext 6, 4, 2, edge launches at ext 0 (64 % 64 == 0)"),
    "fold-24-1x2": ("fold", 20, 24, 1, 2, None, 4, 4, [
        (20, 12, 2, (1, 3, 12), False, {2}),
        (20, 12, 1, (1, 1, 11), False, {1, 2}),
    ], "north rank Mm = 12: (12 + ext) % 4 == 0 blocks the fold at ext 0 and 4"),
    "fold-28-1x2": ("fold", 20, 28, 1, 2, None, 4, 4, [
        (20, 14, 2, (1, 3, 14), False, {2}),
        (20, 14, 2, (1, 1, 13), False, {1, 2}),
    ], "north rank Mm = 14: the fold blocked at ext 2 and 6"),
    "fold-26-1x2": ("fold", 20, 26, 1, 2, None, 4, 4, [
        (20, 13, 2, (1, 3, 13), False, {2}),
        (20, 13, 2, (1, 1, 12), False, {2}),
    ], "the control: odd Mm = 13 never blocks the fold"),
    "fold-96x28-2x2": ("fold", 96, 28, 2, 2, None, 4, 4, [
        (48, 14, 2, (1, 3, 14), True, {2}),
        (48, 14, 2, (1, 3, 14), True, {1, 2}),
        (48, 14, 2, (1, 1, 13), True, {1, 2}),
        (48, 14, 2, (1, 1, 13), True, {1, 2}),
    ], "north-east rank: the east term blocks at ext 6, 4, 2, the north term at 6 and 2, out of phase"),
    "fold-96-2x1-K1": ("fold", 96, 10, 2, 1, "1", 1, 4, [
        (48, 10, 2, (1, 3, 9), True, {2}),
        (48, 10, 2, (1, 3, 9), True, {2}),
    ], "K = 1: no widening, the base mode alone"),
    "fold-96-2x1-K2": ("fold", 96, 10, 2, 1, "2", 2, 4, [
        (48, 10, 2, (1, 3, 9), True, {2}),
        (48, 10, 2, (1, 3, 9), True, {1, 2}),
    ], "K = 2: ext 2 and 0 alternate"),
    "fold-96-2x1-K3": ("fold", 96, 10, 2, 1, "3", 3, 4, [
        (48, 10, 2, (1, 3, 9), True, {2}),
        (48, 10, 2, (1, 3, 9), True, {1, 2}),
    ], "K = 3: ext 4, 2, 0"),
    # ---- a rank without a wall in a closed basin
    "nowall-54x42-3x3": ("kpp", 54, 42, 3, 3, None, 4, 4, [
        (18, 14, 2, (1, 3, 14), False, {2}),
        (18, 14, 2, (1, 3, 14), False, {2}),
        (18, 14, 2, (1, 3, 14), False, {2}),
        (18, 14, 2, (1, 1, 14), False, {2}),
        (18, 14, 0, (1, 1, 14), False, {0}),
        (18, 14, 2, (1, 1, 14), False, {2}),
        (18, 14, 2, (1, 1, 13), False, {1, 2}),
        (18, 14, 2, (1, 1, 13), False, {1, 2}),
        (18, 14, 2, (1, 1, 13), False, {1, 2}),
    ], "centre rank: edge mode 0 without periodic images, no edge strip, four corner exchanges"),
    "nowall-54x42-3x3-n100": ("n100", 54, 42, 3, 3, None, 4, 3, [
        (18, 14, 2, (1, 3, 14), False, {2}),
        (18, 14, 2, (1, 3, 14), False, {2}),
        (18, 14, 2, (1, 3, 14), False, {2}),
        (18, 14, 2, (1, 1, 14), False, {2}),
        (18, 14, 0, (1, 1, 14), False, {0}),
        (18, 14, 2, (1, 1, 14), False, {2}),
        (18, 14, 2, (1, 1, 13), False, {1, 2}),
        (18, 14, 2, (1, 1, 13), False, {1, 2}),
        (18, 14, 2, (1, 1, 13), False, {1, 2}),
    ], "the same at N = 100: segment solvers and v-tiles on ranks with no wall"),
    # ---- 16-column blocks and the omega switch
    "omega-63-2x1": ("kpp", 63, 10, 2, 1, None, 4, 4, [
        (32, 10, 2, (1, 3, 9), True, {2}),
        (31, 10, 2, (1, 3, 9), False, {2}),
    ], "west rank k_omega_seg, east rank the two-pass k_omega, the single domain the segment form"),
    "block-33-2x1-n100": ("n100", 33, 6, 2, 1, None, 2, 3, [
        (17, 6, 2, (1, 3, 5), False, {2}),
        (16, 6, 2, (1, 3, 5), False, {2}),
    ], "N = 100: a segment-solver block of one column next to the rank boundary (west rank)"),
    "block-65-2x1-n100": ("n100", 65, 6, 2, 1, None, 2, 3, [
        (33, 6, 2, (1, 3, 5), True, {2}),
        (32, 6, 2, (1, 3, 5), True, {2}),
    ], "N = 100: k_omega_seg with a third block of one column next to the rank boundary"),
    # ---- the smallest ranks: the 2-deep halo is the neighbour's whole interior; K falls to 1
    "tiny-kpp-12-3x1": ("kpp", 12, 8, 3, 1, None, 1, 4, [
        (4, 8, 2, (1, 3, 7), False, {2}),
        (4, 8, 2, (1, 3, 7), False, {2}),
        (4, 8, 2, (1, 3, 7), False, {2}),
    ], "ranks 4 wide: a neighbour's halo and packed columns are all it owns"),
    "tiny-kpp-12-1x3": ("kpp", 8, 12, 1, 3, None, 1, 4, [
        (8, 4, 2, (1, 3, 4), False, {2}),
        (8, 4, 2, (1, 1, 4), False, {2}),
        (8, 4, 1, (1, 1, 3), False, {1}),
    ], "ranks 4 high; the north rank's (4 + 0) % 4 == 0 blocks the fold"),
    "tiny-kpp-6-3x1": ("kpp", 6, 8, 3, 1, None, 1, 4, [
        (2, 8, 2, (1, 3, 7), False, {2}),
        (2, 8, 2, (1, 3, 7), False, {2}),
        (2, 8, 2, (1, 3, 7), False, {2}),
    ], "ranks 2 wide: the smallest roms_gpu_init accepts, the halo is the neighbour's whole interior"),
    "tiny-kpp-6-1x3": ("kpp", 8, 6, 1, 3, None, 1, 4, [
        (8, 2, 2, None, False, {2}),
        (8, 2, 2, (1, 1, 2), False, {2}),
        (8, 2, 2, (1, 1, 1), False, {2}),
    ], "ranks 2 high: no strip row on the south rank, one on the north rank"),
    "tiny-kpp-5-2x1": ("kpp", 5, 8, 2, 1, None, 1, 4, [
        (3, 8, 2, (1, 3, 7), False, {2}),
        (2, 8, 2, (1, 3, 7), False, {2}),
    ], "uneven smallest split: 3 and 2 columns"),
    "tiny-kpp-5-1x2": ("kpp", 8, 5, 1, 2, None, 1, 4, [
        (8, 3, 2, (1, 3, 3), False, {2}),
        (8, 2, 2, (1, 1, 1), False, {2}),
    ], "uneven smallest split: 3 and 2 rows, one strip row each"),
    "tiny-fil-12-3x1": ("filament", 12, 8, 3, 1, None, 1, 4, [
        (4, 8, 0, (1, 1, 8), False, {0}),
        (4, 8, 0, (1, 1, 8), False, {0}),
        (4, 8, 0, (1, 1, 8), False, {0}),
    ], "periodic ranks 4 wide"),
    "tiny-fil-12-1x3": ("filament", 8, 12, 1, 3, None, 1, 4, [
        (8, 4, 0, (1, 1, 4), False, {0}),
        (8, 4, 0, (1, 1, 4), False, {0}),
        (8, 4, 0, (1, 1, 4), False, {0}),
    ], "periodic ranks 4 high"),
    "tiny-fil-6-3x1": ("filament", 6, 8, 3, 1, None, 1, 4, [
        (2, 8, 0, (1, 1, 8), False, {0}),
        (2, 8, 0, (1, 1, 8), False, {0}),
        (2, 8, 0, (1, 1, 8), False, {0}),
    ], "periodic ranks 2 wide: each halo is a neighbour's whole interior"),
    "tiny-fil-6-1x3": ("filament", 8, 6, 1, 3, None, 1, 4, [
        (8, 2, 0, (1, 1, 2), False, {0}),
        (8, 2, 0, (1, 1, 2), False, {0}),
        (8, 2, 0, (1, 1, 2), False, {0}),
    ], "periodic ranks 2 high"),
    "tiny-fil-5-2x1": ("filament", 5, 8, 2, 1, None, 1, 4, [
        (3, 8, 0, (1, 1, 8), False, {0}),
        (2, 8, 0, (1, 1, 8), False, {0}),
    ], "periodic, 3 and 2 columns: both neighbours of a rank are the other rank"),
    "tiny-fil-5-1x2": ("filament", 8, 5, 1, 2, None, 1, 4, [
        (8, 3, 0, (1, 1, 3), False, {0}),
        (8, 2, 0, (1, 1, 2), False, {0}),
    ], "periodic, 3 and 2 rows"),
    # ---- open edges never fold and take every fast step's exchange (K = 1)
    "open-121-2x1": ("open", 121, 10, 2, 1, None, 1, 4, [
        (61, 10, 1, (2, 3, 9), True, {1}),
        (60, 10, 1, (1, 3, 9), True, {1}),
    ], "east rank: one full strip at the open east edge with a rank boundary to the west"),
    "open-96-2x1": ("open", 96, 10, 2, 1, None, 1, 4, [
        (48, 10, 1, (1, 3, 9), True, {1}),
        (48, 10, 1, (1, 3, 9), True, {1}),
    ], "48-wide ranks with open edges: the edge launches whatever the tiles' start"),
}


def sub_cfg(family, LLm, MMm):
    """The oracle configuration of the family on the global grid."""
    N = FAMILY_N[family]
    if family == "filament":
        return oracle.filament_cfg(LLm=LLm, MMm=MMm, N=N, sizex=200.0 * LLm, sizey=50.0 * MMm, np_xi=1, np_eta=1)
    c = basin_cfg(nonlin=True, LLm=LLm, MMm=MMm, N=N, sizex=2.0e3 * LLm, sizey=2.0e3 * MMm)
    if family == "open":
        c.obc, c.ubind, c.island, c.lmd = 15, 0.1, 1, oracle.LMD_ALL
    elif family != "fold":
        c.lmd, c.surf_flux = oracle.LMD_ALL, 1
    return c


def case_of(cfg):
    """Model.from_case's arguments for the oracle configuration."""
    return dict(case_id=cfg.case_id, LLm=cfg.LLm, MMm=cfg.MMm, N=cfg.N, NT=cfg.NT, salinity=bool(cfg.salinity),
                nonlin_eos=bool(cfg.nonlin_eos), dt=cfg.dt, ndtfast=cfg.ndtfast, sizex=cfg.sizex, sizey=cfg.sizey,
                lmd=cfg.lmd, surf_flux=bool(cfg.surf_flux), obc=cfg.obc, v_sponge=cfg.v_sponge,
                island=bool(cfg.island))


def predicted(name):
    """(K, per-rank tuples) of an entry from the host predicates written out:
    the interval of roms_gpu_init (2K + 2 fits the smallest extent; 1 with
    open edges), s2d_edge_mode on the bounds launch_step2d widens by ext,
    prsgrd_strip_rows, omega_takes_seg."""
    family, LLm, MMm, npx, npe, kenv = ENTRIES[name][:6]
    per = family == "filament"
    ext_x = [romsgpu.rank_extent(LLm, npx, r)[0] for r in range(npx)]
    ext_y = [romsgpu.rank_extent(MMm, npe, r)[0] for r in range(npe)]
    K = 1 if family == "open" else int(kenv or 4)
    while K > 1 and min(ext_x + ext_y) < 2 * K + 2:
        K -= 1
    ranks = []
    for rank in range(npx * npe):
        jn, inn = divmod(rank, npx)
        Lm, Mm = ext_x[inn], ext_y[jn]
        W, E, S, Nw = (not per and inn == 0, not per and inn == npx - 1, not per and jn == 0,
                       not per and jn == npe - 1)

        def mode(ext):
            if not (W or E or S or Nw):
                return 0
            if family == "open":
                return 1
            istrR, iendR = (0 if W else 1 - ext), (Lm + 1 if E else Lm + ext)
            jstrR, jendR = (0 if S else 1 - ext), (Mm + 1 if Nw else Mm + ext)
            t0 = istrR - ((istrR - 1) & 15)   # tile_i0
            fold = ((not E or (iendR - t0) % 64 != 0) and (not W or (istrR - t0) % 64 != 63)
                    and (not Nw or (jendR - jstrR) % 4 != 0))
            return 2 if fold else 1

        jA, jB = (3 if S else 1), (Mm - 1 if Nw else Mm)
        ranks.append((Lm, Mm, mode(0), ((Lm + 59) // 60, jA, jB) if jB >= jA else None, Lm >= 32,
                      {mode(2 * m) for m in range(K)}))
    return K, ranks


def test_table_matches_predicates():
    """Every entry's rank extents (romsgpu.rank_extent), interval and paths
    are those the predicates give, and the entries the sweep is there for
    name what they should."""
    bad = [(n, predicted(n), (e[6], e[8])) for n, e in ENTRIES.items() if predicted(n) != (e[6], e[8])]
    assert not bad, bad
    for n, e in ENTRIES.items():
        assert len(e[8]) == e[3] * e[4] <= 9 and 3 <= e[7] <= 5, n
    modes = {n: [r[5] for r in e[8]] for n, e in ENTRIES.items()}
    for n in ("fold-96-2x1", "fold-128-2x1", "fold-24-1x2", "fold-28-1x2"):
        assert modes[n] == [{2}, {1, 2}], n   # west / south, east / north
    assert modes["fold-26-1x2"] == [{2}, {2}]
    assert modes["fold-96x28-2x2"][3] == {1, 2}
    assert modes["nowall-54x42-3x3"][4] == modes["nowall-54x42-3x3-n100"][4] == {0}
    assert all(e[6] == 1 for n, e in ENTRIES.items() if n.startswith(("tiny", "open")))


ENV_CLEAR = {"ROMS_GPU_S2D_K": None, "ROMS_GPU_PRS_STRIP": None, "ROMS_GPU_S2D_EDGES": None, "ROMS_GPU_T_STRIP": None}


def paths_of(m):
    """What a rank reports after its steps (run_decomposed's probe)."""
    return (m.Lm, m.Mm), m.horizontal_path(), m.fast_step_edge_modes(), m.halo_exchanges()[1]


def wrong_paths(name, got, change=None):
    """The ranks whose probes differ from the entry (change: what a variant's
    environment alters)."""
    family, LLm, MMm, npx, npe, _, K, _, ranks, why = ENTRIES[name]
    bad = []
    for rank, (Lm, Mm, edges, strips, seg, modes) in enumerate(ranks):
        want = ((Lm, Mm), {"edges": edges, "strips": strips, "omega_seg": seg}, modes, K)
        if change:
            want = change(want)
        if got.get(rank) != want:
            bad.append((rank, "got", got.get(rank), "expected", want))
    return bad


@pytest.mark.parametrize("name", list(ENTRIES))
def test_subdomain_bitwise_and_paths(name):
    """(a) every rank of the entry equals the single-domain window bitwise
    after the entry's whole steps; (c) every rank took the paths the entry
    names (asserted first, so a wrong path shows beside the numbers)."""
    family, LLm, MMm, npx, npe, kenv, K, nsteps, ranks, why = ENTRIES[name]
    case = case_of(sub_cfg(family, LLm, MMm))
    got, bitwise = {}, None
    with environ(dict(ENV_CLEAR, ROMS_GPU_S2D_K=kenv)):
        try:
            check_decomposition(case, npx, npe, nsteps=nsteps,
                                probe=lambda m: got.__setitem__(m.inode + m.jnode * npx, paths_of(m)))
        except AssertionError as e:
            bitwise = e
    bad = wrong_paths(name, got)
    assert not bad, (name, why, bad, "and bitwise:", str(bitwise).split("\n")[0] if bitwise else "equal")
    if bitwise is not None:
        raise AssertionError((name, why)) from bitwise


GRIDS = sorted({e[:3] for e in ENTRIES.values()})


@pytest.mark.parametrize("family,LLm,MMm", GRIDS, ids=["%s-%dx%d" % g for g in GRIDS])
def test_subdomain_grid_oracle_rms(family, LLm, MMm):
    """(b) the single-domain run every entry on this grid is compared with
    bitwise: 12 whole steps against the CPU oracle, field RMS within RMS_RUN."""
    cfg = sub_cfg(family, LLm, MMm)
    o = oracle.Oracle(cfg)
    o.init()
    o.step(12)
    with environ(ENV_CLEAR):
        m = romsgpu.Model.from_case(**case_of(cfg))
    try:
        m.step(12)
        m.sync()
        assert o.tindex() == m.t.as_list()
        errs = check_fields(o, m, PROGNOSTIC, LLm, MMm, float("inf"), kind="rms")
    finally:
        m.close()
    tag = "%s %dx%d" % (family, LLm, MMm)
    print(tag, {k: "%.2e" % v for k, v in errs.items()})
    print("%s worst run rms %.3e" % (tag, max(errs.values())))
    bad = [(n, e) for n, e in errs.items() if not e <= RMS_RUN]
    assert not bad, (tag, bad)


# variant -> (environment, what it changes in a rank's expected (extents, path, modes, K))
VARIANTS = {
    "prs_tiles": ({"ROMS_GPU_PRS_STRIP": "0"}, lambda w: (w[0], dict(w[1], strips=None), w[2], w[3])),
    "tracer_strips": ({"ROMS_GPU_T_STRIP": "1"}, None),
    "edge_launches": ({"ROMS_GPU_S2D_EDGES": "1"}, lambda w: (w[0], dict(w[1], edges=1), {1}, w[3])),
}
_DEFAULT_PARTS = {}   # one entry: the table entry last asked for


def run_parts(name, env, change):
    family, LLm, MMm, npx, npe, kenv, _, nsteps = ENTRIES[name][:8]
    case = case_of(sub_cfg(family, LLm, MMm))
    with environ(dict(ENV_CLEAR, ROMS_GPU_S2D_K=kenv, **env)):
        parts, _ = run_decomposed(case, npx, npe, nsteps, fields=BITWISE_FIELDS, probe=paths_of)
    bad = wrong_paths(name, {r: p[5] for r, p in enumerate(parts)}, change)
    assert not bad, (name, ENTRIES[name][9], bad)
    return [p[4] for p in parts]


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", ["strip-kpp-121x20-2x2", "strip-kpp-240-2x1"])
def test_subdomain_variants_bitwise(name, variant):
    """The decomposed run with the prsgrd tiles, the tracer strips or the
    separate edge launches: rank by rank the bits of the default decomposed
    run (test_width_variants_bitwise on ranks)."""
    if name not in _DEFAULT_PARTS:
        _DEFAULT_PARTS.clear()
        _DEFAULT_PARTS[name] = run_parts(name, {}, None)
    ref = _DEFAULT_PARTS[name]
    env, change = VARIANTS[variant]
    got = run_parts(name, env, change)
    assert all(np.isfinite(r[f]).all() for r in ref for f in BITWISE_FIELDS)
    bad = [(rank, f, float(np.nanmax(np.abs(g[f] - r[f])))) for rank, (g, r) in enumerate(zip(got, ref))
           for f in BITWISE_FIELDS if not np.array_equal(g[f], r[f])]
    assert not bad, (name, variant, bad[:8])
