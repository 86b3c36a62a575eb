# das_staged.hip without step A of round 7: the channel-paired kernel's plain loop reads a batch's table row at the top of the batch
# (as the range-checked loop does) instead of requesting it behind the previous batch's rotate-accumulates
import sys
p = sys.argv[1]
s = open(p).read()
old = "constexpr bool AHEAD = MODE == 1 && NL <= 3;"
assert s.count(old) == 1
open(p, "w").write(s.replace(old, "constexpr bool AHEAD = false;"))
