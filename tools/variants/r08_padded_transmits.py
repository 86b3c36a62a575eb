# das_staged.hip without round 8's "real transmits only": the channel-paired kernel's rounds run and stage the transmit count padded
# to a multiple of 4 again (zero phasors over zero windows), as the parent did
import sys
p = sys.argv[1]
s = open(p).read()
for old, new in (
        # the padding transmits are staged as zeros from outside the buffer ...
        ("if (a >= (uint32_t)A) off = STAGE_SKIP;", "if (a >= (uint32_t)A) off = 0x80000000u;"),
        # ... by an offset that a missing odd channel's 2 GiB must not wrap back into the buffer ...
        ("(int)(lane_at + off), 0, 0);", "(int)(off == 0x80000000u ? off : lane_at + off), 0, 0);"),
        # ... and the rounds run the whole group
        ("gr = left < gn ? left : gn;", "gr = gn; (void)left;")):
    assert s.count(old) == 1, old
    s = s.replace(old, new)
open(p, "w").write(s)
