/*
 * ref_noise.cpp -- the noise source of the compiled reference library (oracle/Makefile, target `ref`).
 * TEST INFRASTRUCTURE ONLY; this project's own text.  ref_shim/windows.h renames the reference's rand() calls to
 * ref_rand(), which either passes through to libc rand() (for the known answers recorded after srand(1)) or gives the
 * project's counter stream klatt_noise31(seed, k) -- restated here from its definition (oracle/klatt_oracle.c), the
 * oracle is not linked in.  The state is process-global, like rand()'s: the caller sets (mode, seed, k) before a call
 * into the library, reads k back after it, and serialises.
 */
#include <cstdint>
#include <cstdlib>

static int g_mode = 0;          /* 0 = libc rand(), 1 = counter stream */
static uint32_t g_seed = 0, g_k = 0;

static uint32_t mix(uint32_t x)
{
    x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
    return x;
}

/* s_0 = mix(seed ^ 0x9E3779B9), c = (mix(seed + 0x85EBCA6B) << 1) | 1, s_(n+1) = 1664525 s_n + c; value k = s_(k+1) >> 1 */
static uint32_t noise31(uint32_t seed, uint32_t k)
{
    uint32_t a = 1664525u, c = (mix(seed + 0x85EBCA6Bu) << 1) | 1u, accA = 1u, accC = 0u;
    for (uint64_t n = (uint64_t)k + 1u; n; n >>= 1) {
        if (n & 1u) { accA *= a; accC = accC * a + c; }
        c = (a + 1u) * c; a *= a;
    }
    return (accA * mix(seed ^ 0x9E3779B9u) + accC) >> 1;
}

extern "C" {

void ref_noise_set(int mode, uint32_t seed, uint32_t k) { g_mode = mode; g_seed = seed; g_k = k; }
uint32_t ref_noise_position(void) { return g_k; }
uint32_t ref_noise31(uint32_t seed, uint32_t k) { return noise31(seed, k); }

int ref_rand(void)
{
    if (g_mode == 0) return (rand)();
    return (int)noise31(g_seed, g_k++);
}

}
