/* paired_split.cpp -- prints what bf_kernels.h's split of the channel-paired staged kernel's transmits gives for every padded transmit
 * count and a set of channel chunks: one line "a4 chunk ok g0 g1 passes0 passes1 lds_bytes" each (tests/test_staged_paired_split.py).
 * Host build of the very functions the plan, the launcher and the kernel call. */
#include <cstdio>
#include <cstdlib>
#include "bf_kernels.h"

int main(int argc, char **argv)
{
	for (uint32_t a4 = 4; a4 <= 2u * BF_STAGED_PAIRED_GROUP_MAX + 8u; a4 += 4)
		for (int i = 1; i < argc; i++) {
			const uint32_t chunk = (uint32_t)std::atoi(argv[i]);
			uint32_t g0 = 0, g1 = 0;
			const bool ok = bf_staged_paired_split(a4, chunk, &g0, &g1);
			std::printf("%u %u %d %u %u %u %u %u\n", a4, chunk, ok ? 1 : 0, g0, g1, ok ? bf_staged_paired_passes(g0) : 0u,
			            ok && g1 ? bf_staged_paired_passes(g1) : 0u, ok ? bf_staged_paired_lds_bytes(g0, chunk, a4) : 0u);
		}
	std::printf("max %u budget %u\n", BF_STAGED_PAIRED_GROUP_MAX, BF_STAGED_PAIRED_LDS_BUDGET);
	return 0;
}
