// SHA-256 counter-mode generator: the same stream as the reference's spasm_prng.c, so that seeded runs draw the same
// coefficients (the low-rank mode of the driver) and the same challenges (the rank certificates) as the reference.
#pragma once

#include <cstring>

#include "common.h"
#include "sha256.h"

namespace sh {

struct Prng {
	uint8_t block[44];
	uint8_t hash[32];
	uint32_t prime, mask;
	uint32_t counter;
	int pos;

	static void be32(uint8_t *dst, uint32_t v)
	{
		dst[0] = (uint8_t) (v >> 24);
		dst[1] = (uint8_t) (v >> 16);
		dst[2] = (uint8_t) (v >> 8);
		dst[3] = (uint8_t) v;
	}

	void rehash()
	{
		Sha256 h;
		h.reset();
		h.update(block, 44);
		h.finish(hash);
		counter += 1;
		be32(block + 36, counter);
		pos = 0;
	}

	// spasm_prng_seed (spasm_prng.c:47-63): a 32-byte seed (a SHA-256 digest), the modulus, a sequence number
	void seed_hash(const uint8_t *seed32, i64 p, uint32_t seq)
	{
		std::memset(block, 0, sizeof(block));
		std::memcpy(block, seed32, 32);
		prime = (uint32_t) p;
		i64 m = 1;
		while (m < p)
			m <<= 1;
		mask = (uint32_t) (m - 1);
		be32(block + 32, (uint32_t) p);
		be32(block + 40, seq);
		counter = 0;
		rehash();
	}

	// spasm_prng_seed_simple (spasm_prng.c:68-76): a 64-bit seed in the first two big-endian words of the 32-byte seed
	void seed(i64 p, uint64_t s, uint32_t seq)
	{
		uint8_t s32[32] = {0};
		be32(s32 + 0, (uint32_t) (s & 0xffffffffu));
		be32(s32 + 4, (uint32_t) (s >> 32));
		seed_hash(s32, p, seq);
	}

	uint32_t next_u32()
	{
		if (pos == 8)
			rehash();
		const uint8_t *b = hash + 4 * pos;
		pos += 1;
		return ((uint32_t) b[0] << 24) | ((uint32_t) b[1] << 16) | ((uint32_t) b[2] << 8) | b[3];
	}

	spasm_ZZp next_zp()
	{
		for (;;) {
			uint32_t x = next_u32() & mask;
			if (x < prime)
				return zp_init(prime, x);
		}
	}
};

}  // namespace sh
