"""Run-length patterns for the moment sweep's round loop (test helper).

tests/_ragged.py PATTERNS stops at two software-pipelined rounds (lmin4 <= 11).
lanes_fast.h lf_moments_pre alternates two register sets over the rounds, takes
its first two rounds' loads from the caller (issued a step earlier) and
leaves its loop at either parity of the round count; these patterns reach
three to six rounds with every remainder and tail.  With 12 groups on one
slice and MC_LANES_REP=1 a lane's run is one group (rep = 1, one register
slot); as planned the groups are split over four lanes each (rep = 4: runs of
12..26, no or one round).

name -> (observations per group, lmin4, full rounds, lmax, N) for one lane
per group.  round6 is the round count of the benchmark's shapes.
"""
from _ragged import _cyc

ROUNDS = {
    # 3 rounds: the loop runs once and ends after set A
    "round3": (_cyc(12, lambda i: 48 + i % 8), 12, 3, 55, 610),
    # 4 rounds: the loop runs once, the last round is set B's; an empty group
    "round4": ([0] + _cyc(11, lambda i: 64 + i % 8), 16, 4, 71, 735),
    "round5": (_cyc(12, lambda i: 80 + i % 8), 20, 5, 87, 994),
    "round6": ([0] + _cyc(11, lambda i: 96 + i % 8), 24, 6, 103, 1087),
}
NAMES = sorted(ROUNDS)
PLANNED_REP = 4     # plan_lanes.hip plan_lanes: min(16, 64 / 16) lanes per parameter for 12 groups
