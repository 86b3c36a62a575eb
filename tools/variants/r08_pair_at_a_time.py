# das_staged.hip without round 8's runs of channel pairs: the channel-paired kernel chooses its case (skip / plain / range-checked)
# anew for every pair, so the three cases meet after every pair and every pair requests its own first windows
import sys
p = sys.argv[1]
s = open(p).read()
for old, new in (("else if (next_mode == MODE) stage_load(", "else if (false) stage_load("),
                 ("} while (mode == MODE);", "} while (false);")):
    assert s.count(old) == 1, old
    s = s.replace(old, new)
open(p, "w").write(s)
