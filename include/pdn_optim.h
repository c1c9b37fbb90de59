/* Optimizer extensions of the pdnhip C ABI (csrc/optim.hip), exported by libpdnhip.so beside include/pdn_hip.h and
 * bound by pydynet_amd/_lib.py with it.  Conventions (status codes, pdn_last_error, streams) are the core header's.
 *
 * Why a header and a prefix (pdnx_) of their own: the tests hold include/pdn_hip.h, the library's pdn_* exports and the
 * registry of the host emulation (EmulatedLib and NOT_EMULATED in tests/abi_emulator/__init__.py) equal, and that registry
 * is an existing test file which a change that only adds a feature leaves as it is.  The same three-way equality is
 * held for this header by tests/test_optim_abi_cpu.py: the library's pdnx_* exports, and the emulation in
 * tests/abi_emulator/_optim.py with its own NOT_EMULATED.  Moving the entries into the core header later is a rename
 * and two registry lines. */
#ifndef PDN_OPTIM_H
#define PDN_OPTIM_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---- Global-norm gradient clipping over the same chunk table (csrc/optim.hip).  These extend
 * optim/optimizer.py:185-196; the reference has no counterpart.  Statement: pydynet_amd/optim/clip.py.
 * partials_dev: double[nchunks], one sum of squares per chunk, reduced in a fixed order (bit-reproducible).
 * ctl_dev: float[4] = {norm, coef, skip (0 or 1), skipped steps}; norm = |grad_scale| * sqrt(sum g^2),
 * coef = min(1, max_norm / (norm + 1e-6)); a non-finite norm gives coef 0, skip 1 and ctl[3] += 1 (ctl[3]
 * persists across calls: the caller zeroes it once).  Gradients are read, never written. */
int pdnx_grad_norm_multi_f32(const int64_t* chunk_table_dev, int nchunks, float grad_scale, float max_norm,
                            double* partials_dev, float* ctl_dev, void* stream);      /* max_norm <= 0: measure only, coef 1 */
/* g *= ctl[1] over the table (for optimizers that do not take the coefficient themselves); nothing is written
 * when ctl[2] != 0 */
int pdnx_grad_scale_multi_f32(const int64_t* chunk_table_dev, int nchunks, const float* ctl_dev, void* stream);

/* ---- Adam.step with the clip coefficient and / or decoupled weight decay (csrc/optim.hip); these too extend
 * optim/optimizer.py:185-196 and have no counterpart in the reference.  pdn_adam_multi_f32's arithmetic with
 * g*grad_scale replaced by g*grad_scale*ctl[1], and the whole update skipped (p, m, v untouched) when ctl[2] != 0;
 * decoupled: p -= lr_wd * p first (lr_wd = lr * weight_decay) and no weight_decay * p in the gradient.
 * The tick form is replayable from a hipGraph like pdn_adam_multi_tick_f32: state_dev = {t, lr} doubles, one launch
 * finishes the norm, writes step_dev = {lr*a_t, lr*weight_decay} and advances t (also when the update is skipped).
 * Its ctl_dev may be NULL as well (no clipping: tick + update); otherwise partials_dev is required.
 * 1 - beta (and the betas of a_t in the tick form) are formed from beta ROUNDED TO SEVEN DECIMALS: 0.999 arrives as the
 * float 0.99900001287, and 1 minus that would miss 0.001 by 1.3e-5 of its value.  This is a guess at what the caller
 * wrote: a beta with more than seven decimals is altered by up to 5e-8 (under one float32 ulp), and the result differs
 * from pdn_adam_multi_tick_f32, which uses (double)beta and 1.f - beta. */
int pdnx_adam_multi_clip_f32(const int64_t* chunk_table_dev, int nchunks, float step, float lr_wd, float beta1, float beta2,
                            float eps, float weight_decay, float grad_scale, int decoupled, const float* ctl_dev /* may be NULL */,
                            void* stream);
int pdnx_adam_multi_clip_tick_f32(const int64_t* chunk_table_dev, int nchunks, double* state_dev, float* step_dev /* [2]: step, lr_wd */,
                                 float beta1, float beta2, float eps, float weight_decay, float grad_scale, float max_norm,
                                 int decoupled, double* partials_dev, float* ctl_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif
