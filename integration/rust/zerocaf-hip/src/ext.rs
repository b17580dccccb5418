//! Additive entry points beyond the 0.6 table (`include/zerocaf_hip_ext.h` and `zerocaf_hip_ext_sum.h`, which it includes).
//!
//! `ffi.rs` is the rendering of `zerocaf_hip.h` and stays exactly that; calls declared in the second header are bound here,
//! with their own `extern "C"` block and a safe wrapper each.

use std::os::raw::c_int;

use zerocaf::ristretto::{CompressedRistretto, RistrettoPoint};
use zerocaf::scalar::Scalar;

use super::ffi::ZcCtx;
use super::{bytes32, check, flat_ris, flat_sc, HipBackend, Result};

extern "C" {
    /// `out32[i] = RistrettoPoint(2 * P_i).compress()`; see `zerocaf_hip_ext.h`.
    pub fn zc_ris_double_and_compress(ctx: *mut ZcCtx, p: *const u64, out32: *mut u8, n: usize) -> c_int;
    /// `out32 = compress(b * B + sum_i sum_j w_ij * decompress(in32[i][j]))`, one MSM over all rows; see `zerocaf_hip_ext_sum.h`.
    pub fn zc_ris_lincomb_sum(ctx: *mut ZcCtx, in32: *const u8, scalars: *const u64, terms: usize, base_scalars: *const u64, weights: *const u64, out32: *mut u8, ok: *mut u8, n: usize) -> c_int;
}

impl HipBackend {
    /// `RistrettoPoint(p.0.double()).compress()` for every point, without a square root: the rows of the batch share
    /// inversions.  `compress(k * P)` for a point of order L is this call on `(k * 2^-1 mod L) * P`.  A point of E[8]
    /// gives 32 zero bytes, as the reference's composition does.
    pub fn ris_double_and_compress(&self, p: &[RistrettoPoint]) -> Result<Vec<CompressedRistretto>> {
        let (fp, n) = (flat_ris(p), p.len());
        let mut out = vec![0u8; n * 32];
        if n > 0 {
            check(unsafe { zc_ris_double_and_compress(self.ctx, fp.as_ptr(), out.as_mut_ptr(), n) })?;
        }
        Ok(out.chunks_exact(32).map(|c| CompressedRistretto(bytes32(c))).collect())
    }

    /// The weighted sum of all rows of a wire-format batch as one MSM: `(b * RISTRETTO_BASEPOINT + sum_i sum_j w_ij *
    /// cs[i][j].decompress()?).compress()` with `w_ij = weights[i] * ks[i][j] mod L` and `b = sum_i weights[i] * base[i] mod L`,
    /// every scalar read by value.  A row with a term that does not decode has `false` in the mask and is left out of both
    /// sums.  A batch verifies when the mask is all `true` and the encoding is 32 zero bytes (a subtracted term is `L - c`;
    /// weights of 128 random bits suffice).
    pub fn ris_lincomb_sum(&self, cs: &[Vec<CompressedRistretto>], ks: &[Vec<Scalar>], base: Option<&[Scalar]>, weights: Option<&[Scalar]>) -> Result<(CompressedRistretto, Vec<bool>)> {
        assert_eq!(cs.len(), ks.len());
        let n = cs.len();
        let t = cs.first().map_or(1, |c| c.len());
        let mut flat: Vec<u8> = Vec::with_capacity(n * t * 32);
        let mut fk = Vec::with_capacity(n * t * 5);
        for (c, k) in cs.iter().zip(ks) {
            assert!(c.len() == t && k.len() == t);
            flat.extend(c.iter().flat_map(|e| e.0.iter().copied()));
            fk.extend(flat_sc(k));
        }
        let per_row = |v: Option<&[Scalar]>| {
            v.map(|b| {
                assert_eq!(b.len(), n);
                flat_sc(b)
            })
        };
        let (fb, fz) = (per_row(base), per_row(weights));
        let (mut out, mut ok) = ([0u8; 32], vec![0u8; n]);
        if n > 0 {
            let pb = fb.as_ref().map_or(std::ptr::null(), |b| b.as_ptr());
            let pz = fz.as_ref().map_or(std::ptr::null(), |z| z.as_ptr());
            check(unsafe { zc_ris_lincomb_sum(self.ctx, flat.as_ptr(), fk.as_ptr(), t, pb, pz, out.as_mut_ptr(), ok.as_mut_ptr(), n) })?;
        }
        Ok((CompressedRistretto(out), ok.iter().map(|&o| o != 0).collect()))
    }
}
