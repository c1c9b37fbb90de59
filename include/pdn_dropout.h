/* Dropout with the mask drawn on the device -- nn.Dropout(generator=...), fused.dropout / fused.dropout_add, the embedding
 * and residual dropout of Llama: extensions of the pdnhip C ABI (csrc/dropout.hip), exported by libpdnhip.so beside
 * include/pdn_hip.h and bound by pydynet_amd/_lib.py with it.  Conventions (status codes, pdn_last_error, streams) are the
 * core header's.
 *
 * Why a header and a prefix (pdnd_) of their own: as for include/pdn_stopseq.h and the headers before it -- the tests hold
 * each header, the library's exports under its prefix and the closed registry of the host emulation equal.  This header is
 * listed in _lib.DROPOUT_HEADER_PATHS and held to the same three-way equality by tests/test_dropout_abi_cpu.py: the
 * library's pdnd_* exports, and the emulation in tests/abi_emulator/_dropout.py with its own NOT_EMULATED.
 *
 * Statement: pydynet_amd/core/fused/dropout.py (the reference's dropout, nn/modules/dropout.py, draws np.random numbers on
 * the host: no entry below has a counterpart).  The generator is Philox4x32-10.  state: two 64-bit words in device memory,
 * seed and offset.  slot: two 64-bit words in device memory owned by the caller's tape node, the (seed, o) a call claimed.
 * Element i of a call over n elements uses word i % 4 of the block for counter (lo32(c), hi32(c), 0, 0), c = o + i / 4
 * (mod 2^64), and key (lo32(seed), hi32(seed)); it is dropped iff word < floor(p * 2^32), 0 <= p < 1 with float(p) < 1.
 * A kept element is x * s, s = 1.0f / (1.0f - (float)p): one fp32 multiply; a dropped one is exactly 0.
 * Nothing is allocated or read back inside a call and there are no atomics; (seed, o) reach the kernels through the slot
 * alone, so a step that contains a claim and its forward / backward replays from a hipGraph, every replay with a fresh
 * mask.  x / y (and dy / dx) may be the same array.  Each launching entry counts once in launch counter slot 54. */
#ifndef PDN_DROPOUT_H
#define PDN_DROPOUT_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* state[0] = seed, state[1] = offset: one launch, stream-ordered behind the calls queued before it (no counterpart). */
int pdnd_rng_set(int64_t* state, int64_t seed, int64_t offset, void* stream);
/* The claim of a call over n >= 0 elements: slot[0] = state[0], slot[1] = state[1], state[1] += ceil(n / 4).  One launch
 * of one thread (no counterpart). */
int pdnd_rng_claim(int64_t* state, int64_t* slot, int64_t n, void* stream);
/* y[i] = kept(i) ? x[i] * s : 0 for i < n, the mask from slot (no counterpart). */
int pdnd_dropout_fwd_f32(const float* x, float* y, int64_t n, double p, const int64_t* slot, void* stream);
/* dx[i] = kept(i) ? dy[i] * s : 0: the same kernel, named for the direction; the slot is the forward's (no counterpart). */
int pdnd_dropout_bwd_f32(const float* dy, float* dx, int64_t n, double p, const int64_t* slot, void* stream);
/* out[i] = residual[i] + (kept(i) ? x[i] * s : 0): the multiply and the add are two fp32 operations, never an fma.  The
 * backward for x is pdnd_dropout_bwd_f32; the residual's gradient is dy itself (no counterpart). */
int pdnd_dropout_add_fwd_f32(const float* x, const float* residual, float* out, int64_t n, double p, const int64_t* slot,
                             void* stream);

#ifdef __cplusplus
}
#endif
#endif
