"""Run-length patterns for the end of the moment sweep (test helper).

After a run's last full 16-element round lanes_fast.h lf_moments_pre /
lf_moments sum the whole float4 groups below lmin4 (up to three) and then the
masked groups up to the slot's longest run.  tests/_lf_rounds.py's patterns
all have lmin4 divisible by four, so at three or more rounds the pinned round
loop never met a whole group after it; these patterns put zero to three
there at every count of rounds from one to six (no, one and two loop trips,
left at either parity: the idle register set is A or B), with tails from
nothing to more groups than a register set of four would hold.  (A prefetch
of these groups into the idle set was built and measured on them and did not
pay: DESIGN 3.3; the patterns hold whatever form the end takes.)

With 12 groups on one slice and MC_LANES_REP=1 a lane's run is one group
(rep = 1, one register slot).

name -> (observations per group, lmin4, full rounds, whole groups past the
last round, lmax); the tail is lmax - 4 lmin4 elements, the groups past the
last round are ceil(lmax / 4) - 4 rounds.  ORDERS: the data orders a pattern
is run at.
"""
from _ragged import _cyc

ENDS = {
    # the benchmark's own runs: six rounds, one whole group, one masked element
    "bench": ([100, 101] * 6, 25, 6, 1, 101),
    # one round: the loop is not entered; an empty group
    "r1_rem3": ([0] + [28] * 11, 7, 1, 3, 28),
    # two rounds (no loop trip, set A idle): tails of 3 elements, of a whole group
    # (a shortest run of 41, not divisible by four), and 3 + 2 groups
    "r2_tail3": (_cyc(12, lambda i: 32 + i % 4), 8, 2, 0, 35),
    "r2_rem2_grp": (_cyc(12, lambda i: 41 + i % 4), 10, 2, 2, 44),
    "r2_rem3_long": (_cyc(12, lambda i: 44 + i % 9), 11, 2, 3, 52),
    # three rounds (one trip, set B idle): a tail of two groups; 3 + 3 groups
    "r3_rem1_two": (_cyc(12, lambda i: 52 + i % 9), 13, 3, 1, 60),
    "r3_rem3_long": (_cyc(12, lambda i: 60 + i % 11), 15, 3, 3, 70),
    # four rounds (one trip, set A idle): a tail of five groups; one element
    "r4_long": (_cyc(12, lambda i: 64 + (3 * i) % 19), 16, 4, 0, 82),
    "r4_rem3_one": ([76, 77] * 6, 19, 4, 3, 77),
    # five rounds (two trips, set B idle): no tail, an empty group; 3 elements
    "r5_rem2": ([0] + [88] * 11, 22, 5, 2, 88),
    "r5_tail3": (_cyc(12, lambda i: 80 + i % 4), 20, 5, 0, 83),
    # six rounds and nothing after them: the tile ends with the last round
    "r6_exact": ([96] * 12, 24, 6, 0, 96),
}
NAMES = sorted(ENDS)
ORDERS = {n: ("sorted",) if k % 2 else ("shuffled",) for k, n in enumerate(NAMES)}
ORDERS["bench"] = ("sorted", "shuffled")
CASES = [(n, o) for n in NAMES for o in ORDERS[n]]
SET_GROUPS = 4      # float4 groups of a register set
