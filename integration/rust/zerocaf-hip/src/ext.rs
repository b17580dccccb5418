//! Additive entry points beyond the 0.6 table (`include/zerocaf_hip_ext.h`).
//!
//! `ffi.rs` is the rendering of `zerocaf_hip.h` and stays exactly that; calls declared in the second header are bound here,
//! with their own `extern "C"` block and a safe wrapper each.

use std::os::raw::c_int;

use zerocaf::ristretto::{CompressedRistretto, RistrettoPoint};

use super::ffi::ZcCtx;
use super::{bytes32, check, flat_ris, HipBackend, Result};

extern "C" {
    /// `out32[i] = RistrettoPoint(2 * P_i).compress()`; see `zerocaf_hip_ext.h`.
    pub fn zc_ris_double_and_compress(ctx: *mut ZcCtx, p: *const u64, out32: *mut u8, n: usize) -> c_int;
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
}
