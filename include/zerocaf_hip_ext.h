/*
 * zerocaf_hip_ext.h -- additive entry points beyond the 0.6 table.
 *
 * zerocaf_hip.h is the 0.6 ABI: 92 entry points, mirrored one to one by the generated bindings.  Calls added after it are
 * declared here.  They live in the same libraries, follow the same conventions (status codes, host or device arrays, the
 * context's stream, zero decided by value: see zerocaf_hip.h) and leave zc_version() as it is.  Plain C11.
 */
#ifndef ZEROCAF_HIP_EXT_H
#define ZEROCAF_HIP_EXT_H

#include "zerocaf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out32[i] = RistrettoPoint(2 * P_i).compress(), bit-identical to the reference's Double (src/edwards.rs:579-592) followed by
 * compress (src/ristretto.rs:398-425) for every P on the curve, in any coordinates (X:Y:Z:T), any coset of the subgroup.
 * The encoding of a doubled point needs no square root, only the inverse of the product w = (2XY)(Y^2 + X^2)(Z^2 + dT^2)
 * (Z^2 - dT^2), and the rows of a batch share inversions: about 32 field multiplications per row where zc_ris_compress
 * spends about 265.  A caller who controls the scalar multiplies by k/2 mod L (zc_sc_muladd with b = 2^-1 mod L; points of
 * order L only) and gets compress(k * P) from this call.
 *   - A row on the curve gets the reference's bytes.
 *   - A row whose w is 0 mod p BY VALUE gets 32 zero bytes and is left out of the shared product: the eight points of E[8]
 *     (the reference's composition returns 32 zero bytes there too), a record with Z = 0 mod p that keeps T Z = X Y, and any
 *     garbage that lands there.  The same rule as zc_fe_invert and zc_ed_to_affine.
 *   - A row that is not a curve point gets bytes that are deterministic and the same in every launch form (any batch size,
 *     any chunking): garbage in, garbage out, for its own row only.  No row changes another row's result.
 *   - n == 0: ZC_OK, nothing written.  p or out32 NULL: ZC_ERR_BAD_ARG ("null pointer: p", "null pointer: out32"), checked
 *     before n == 0 and before the context ("null context").
 *   - Both arrays in host memory (staged in chunks, synchronous, sharded over the devices of a multi-device context) or both
 *     on one device of the context (used in place, asynchronous on the context's stream); anything else is
 *     ZC_ERR_MIXED_MEM.  Device arrays need 8-byte alignment only.
 *   - out32 must not overlap p.  The call writes rows 0 .. n-1 of out32 and nothing else. */
int zc_ris_double_and_compress(zc_ctx *ctx, const uint64_t *p, uint8_t *out32, size_t n);

#ifdef __cplusplus
}
#endif

/* Calls that reduce a whole batch to one result have a header of their own, which comes in with this one. */
#include "zerocaf_hip_ext_sum.h"
#include "zerocaf_hip_ext_hash.h"
#include "zerocaf_hip_ext_shared.h"
#include "zerocaf_hip_ext_shared_lincomb.h"
#include "zerocaf_hip_ext_gens.h"
#include "zerocaf_hip_ext_sum_rows.h"

#endif /* ZEROCAF_HIP_EXT_H */
