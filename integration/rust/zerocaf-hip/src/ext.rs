//! Additive entry points beyond the 0.6 table (`include/zerocaf_hip_ext.h` and `zerocaf_hip_ext_sum.h` / `zerocaf_hip_ext_hash.h`,
//! which it includes).  The calls with one scalar for a whole batch (`zerocaf_hip_ext_shared.h`, included likewise) and with one
//! scalar vector for a whole batch (`zerocaf_hip_ext_shared_lincomb.h`) follow; the generator sets (`zerocaf_hip_ext_gens.h`) are
//! at the end, before the bounded discrete logs and the scalar vector ops, which have headers of their own (`zerocaf_hip_dlog.h`,
//! `zerocaf_hip_scvec.h`).
//!
//! `ffi.rs` is the rendering of `zerocaf_hip.h` and stays exactly that; calls declared in the second header are bound here,
//! with their own `extern "C"` block and a safe wrapper each.

use std::os::raw::c_int;

use zerocaf::edwards::EdwardsPoint;
use zerocaf::ristretto::{CompressedRistretto, RistrettoPoint};
use zerocaf::scalar::Scalar;

use super::ffi::ZcCtx;
use super::{bytes32, check, flat_ed, flat_ris, flat_sc, masked, unflat_ed, unflat_sc, HipBackend, Result};

extern "C" {
    /// `out32[i] = RistrettoPoint(2 * P_i).compress()`; see `zerocaf_hip_ext.h`.
    pub fn zc_ris_double_and_compress(ctx: *mut ZcCtx, p: *const u64, out32: *mut u8, n: usize) -> c_int;
    /// `out32 = compress(b * B + sum_i sum_j w_ij * decompress(in32[i][j]))`, one MSM over all rows; see `zerocaf_hip_ext_sum.h`.
    pub fn zc_ris_lincomb_sum(ctx: *mut ZcCtx, in32: *const u8, scalars: *const u64, terms: usize, base_scalars: *const u64, weights: *const u64, out32: *mut u8, ok: *mut u8, n: usize) -> c_int;
    /// `out64[i] = SHA-512(prefix || parts[0][i] || parts[1][i] || ...)`; see `zerocaf_hip_ext_hash.h`.
    pub fn zc_sha512_rows(ctx: *mut ZcCtx, prefix: *const u8, prefix_len: usize, parts: *const *const u8, part_len: *const usize, nparts: usize, out64: *mut u8, n: usize) -> c_int;
    /// `out[i]` = that digest as a little-endian integer mod L, five limbs: `zc_sc_from_bytes_wide` without the digest in memory.
    pub fn zc_sc_from_sha512(ctx: *mut ZcCtx, prefix: *const u8, prefix_len: usize, parts: *const *const u8, part_len: *const usize, nparts: usize, out: *mut u64, n: usize) -> c_int;
    /// `out[i]` = `from_uniform_bytes` of that digest, twenty limbs: `zc_ris_from_uniform_bytes` likewise.
    pub fn zc_ris_from_sha512(ctx: *mut ZcCtx, prefix: *const u8, prefix_len: usize, parts: *const *const u8, part_len: *const usize, nparts: usize, out: *mut u64, n: usize) -> c_int;
    /// `out[i] = k * P_i` for ONE scalar `k` (five words in host memory); see `zerocaf_hip_ext_shared.h`.
    pub fn zc_ed_scalar_mul_shared(ctx: *mut ZcCtx, p: *const u64, k: *const u64, out: *mut u64, n: usize) -> c_int;
    /// `out32[i] = compress(k * decompress(in32[i]))` for ONE scalar `k` (five words in host memory); see `zerocaf_hip_ext_shared.h`.
    pub fn zc_ris_mul_shared(ctx: *mut ZcCtx, in32: *const u8, k: *const u64, out32: *mut u8, ok: *mut u8, n: usize) -> c_int;
    /// `out[i] = sum_j k_j * P_ij` for ONE scalar vector `k` (`terms * 5` words in host memory); see `zerocaf_hip_ext_shared_lincomb.h`.
    pub fn zc_ed_lincomb_shared(ctx: *mut ZcCtx, points: *const u64, k: *const u64, terms: usize, out: *mut u64, n: usize) -> c_int;
    /// `out32[i] = compress(sum_j k_j * decompress(in32[i][j]))` for ONE scalar vector `k`; see `zerocaf_hip_ext_shared_lincomb.h`.
    pub fn zc_ris_lincomb_shared(ctx: *mut ZcCtx, in32: *const u8, k: *const u64, terms: usize, out32: *mut u8, ok: *mut u8, n: usize) -> c_int;
    /// A generator set of `count` = 1..8 points with a comb table each, on every device of the context; see `zerocaf_hip_ext_gens.h`.
    pub fn zc_gens_create(ctx: *mut ZcCtx, points: *const u64, count: usize, id_out: *mut u64) -> c_int;
    /// Frees the set after the context's streams have drained.
    pub fn zc_gens_destroy(ctx: *mut ZcCtx, id: u64) -> c_int;
    /// `out[i] = sum_j scalars[i][j] * G_j` over the set `id`: 33 mixed additions per term.
    pub fn zc_ed_mul_gens(ctx: *mut ZcCtx, id: u64, scalars: *const u64, out: *mut u64, n: usize) -> c_int;
    /// `out32[i]` = the Ristretto encoding of that sum.
    pub fn zc_ris_mul_gens_compress(ctx: *mut ZcCtx, id: u64, scalars: *const u64, out32: *mut u8, n: usize) -> c_int;
    /// `out[i] = points[i][0] + points[i][1] + ...` over rows of `terms` points; see `zerocaf_hip_ext_sum_rows.h`.
    pub fn zc_ed_sum_rows(ctx: *mut ZcCtx, points: *const u64, terms: usize, out: *mut u64, n: usize) -> c_int;
    /// `out32[i] = compress(sum_j decompress(in32[i][j]))`; `ok` may be null.
    pub fn zc_ris_sum_rows(ctx: *mut ZcCtx, in32: *const u8, terms: usize, out32: *mut u8, ok: *mut u8, n: usize) -> c_int;
}

/// The message arguments of the three SHA-512 calls from `parts[j]` = n rows of `part_len[j]` contiguous bytes: (pointers, lengths, n).
fn hash_parts(parts: &[(&[u8], usize)]) -> (Vec<*const u8>, Vec<usize>, usize) {
    assert!(!parts.is_empty() && parts.len() <= 4, "1..4 parts");
    let n = parts[0].0.len() / parts[0].1.max(1);
    for (bytes, len) in parts {
        assert!(*len >= 1 && bytes.len() == n * len, "every part holds n rows of its length");
    }
    (parts.iter().map(|p| p.0.as_ptr()).collect(), parts.iter().map(|p| p.1).collect(), n)
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

    /// SHA-512 of `prefix || parts[0][i] || parts[1][i] || ...` for every row: `parts[j]` is (n rows of `len` contiguous bytes, `len`),
    /// 1..4 parts, `prefix` at most 256 bytes.  64 bytes per row, as the `sha2` crate's `Sha512::digest` returns them.
    pub fn sha512_rows(&self, prefix: &[u8], parts: &[(&[u8], usize)]) -> Result<Vec<[u8; 64]>> {
        let (ptrs, lens, n) = hash_parts(parts);
        let mut out = vec![0u8; n * 64];
        if n > 0 {
            check(unsafe { zc_sha512_rows(self.ctx, prefix.as_ptr(), prefix.len(), ptrs.as_ptr(), lens.as_ptr(), lens.len(), out.as_mut_ptr(), n) })?;
        }
        Ok(out.chunks_exact(64).map(|c| { let mut d = [0u8; 64]; d.copy_from_slice(c); d }).collect())
    }

    /// Hash-to-scalar: the SHA-512 digest of every row read as a little-endian 512-bit integer mod L, as five canonical limbs
    /// per row (the layout of `Scalar`'s limbs); the digest stays in registers.
    pub fn sc_from_sha512(&self, prefix: &[u8], parts: &[(&[u8], usize)]) -> Result<Vec<[u64; 5]>> {
        let (ptrs, lens, n) = hash_parts(parts);
        let mut out = vec![0u64; n * 5];
        if n > 0 {
            check(unsafe { zc_sc_from_sha512(self.ctx, prefix.as_ptr(), prefix.len(), ptrs.as_ptr(), lens.as_ptr(), lens.len(), out.as_mut_ptr(), n) })?;
        }
        Ok(out.chunks_exact(5).map(|c| [c[0], c[1], c[2], c[3], c[4]]).collect())
    }

    /// Hash-to-group: `RistrettoPoint::from_uniform_bytes` of every row's SHA-512 digest, as twenty limbs per row (X, Y, Z, T).
    pub fn ris_from_sha512(&self, prefix: &[u8], parts: &[(&[u8], usize)]) -> Result<Vec<[u64; 20]>> {
        let (ptrs, lens, n) = hash_parts(parts);
        let mut out = vec![0u64; n * 20];
        if n > 0 {
            check(unsafe { zc_ris_from_sha512(self.ctx, prefix.as_ptr(), prefix.len(), ptrs.as_ptr(), lens.as_ptr(), lens.len(), out.as_mut_ptr(), n) })?;
        }
        Ok(out.chunks_exact(20).map(|c| { let mut p = [0u64; 20]; p.copy_from_slice(c); p }).collect())
    }

    /// `p[i] * k` for every point and ONE scalar (a view key, an OPRF key): the same group elements as `scalar_mul` with `k`
    /// in every row -- equal under `==`, identical encodings, another projective representative -- on a schedule recoded
    /// once on the host.  The running time depends on `k`.
    pub fn ed_scalar_mul_shared(&self, p: &[EdwardsPoint], k: &Scalar) -> Result<Vec<EdwardsPoint>> {
        let (fp, n) = (flat_ed(p), p.len());
        let mut out = vec![0u64; n * 20];
        if n > 0 {
            check(unsafe { zc_ed_scalar_mul_shared(self.ctx, fp.as_ptr(), k.0.as_ptr(), out.as_mut_ptr(), n) })?;
        }
        Ok(unflat_ed(&out))
    }

    /// `(c[i].decompress()? * k).compress()` for every encoding and ONE scalar, byte-identical to `ris_roundtrip_mul` with `k`
    /// in every row; `None` where an encoding does not decode.  No square root on the way out: the call multiplies by
    /// `k / 2 mod L` and encodes the double.
    pub fn ris_mul_shared(&self, c: &[CompressedRistretto], k: &Scalar) -> Result<Vec<Option<CompressedRistretto>>> {
        let flat: Vec<u8> = c.iter().flat_map(|e| e.0.iter().copied()).collect();
        let n = c.len();
        let (mut out, mut ok) = (vec![0u8; n * 32], vec![0u8; n]);
        if n > 0 {
            check(unsafe { zc_ris_mul_shared(self.ctx, flat.as_ptr(), k.0.as_ptr(), out.as_mut_ptr(), ok.as_mut_ptr(), n) })?;
        }
        let enc: Vec<CompressedRistretto> = out.chunks_exact(32).map(|b| CompressedRistretto(bytes32(b))).collect();
        Ok(masked(enc, &ok))
    }

    /// `sum_j k[j] * p[i][j]` for every row and ONE scalar vector (ElGamal decryption under one key as `(1, -x)`, the Lagrange
    /// coefficients of a threshold decryption, `(u^-1, u)` of a generator folding): the same group elements as `ed_lincomb`
    /// with `k` in every row, on one schedule merged from the terms' recodings on the host.  The running time depends on `k`.
    pub fn ed_lincomb_shared(&self, p: &[Vec<EdwardsPoint>], k: &[Scalar]) -> Result<Vec<EdwardsPoint>> {
        let (n, t) = (p.len(), k.len());
        assert!(p.iter().all(|row| row.len() == t), "one point per scalar in every row");
        let fp: Vec<u64> = p.iter().flat_map(|row| flat_ed(row)).collect();
        let fk = flat_sc(k);
        let mut out = vec![0u64; n * 20];
        if n > 0 {
            check(unsafe { zc_ed_lincomb_shared(self.ctx, fp.as_ptr(), fk.as_ptr(), t, out.as_mut_ptr(), n) })?;
        }
        Ok(unflat_ed(&out))
    }

    /// `(sum_j c[i][j].decompress()? * k[j]).compress()` for every row and ONE scalar vector, byte-identical to `ris_lincomb`
    /// without a base term and with `k` in every row; `None` where a term does not decode.  No basepoint term: pass the
    /// encoding of the basepoint as a term.
    pub fn ris_lincomb_shared(&self, c: &[Vec<CompressedRistretto>], k: &[Scalar]) -> Result<Vec<Option<CompressedRistretto>>> {
        let (n, t) = (c.len(), k.len());
        assert!(c.iter().all(|row| row.len() == t), "one encoding per scalar in every row");
        let flat: Vec<u8> = c.iter().flat_map(|row| row.iter().flat_map(|e| e.0.iter().copied())).collect();
        let fk = flat_sc(k);
        let (mut out, mut ok) = (vec![0u8; n * 32], vec![0u8; n]);
        if n > 0 {
            check(unsafe { zc_ris_lincomb_shared(self.ctx, flat.as_ptr(), fk.as_ptr(), t, out.as_mut_ptr(), ok.as_mut_ptr(), n) })?;
        }
        let enc: Vec<CompressedRistretto> = out.chunks_exact(32).map(|b| CompressedRistretto(bytes32(b))).collect();
        Ok(masked(enc, &ok))
    }

    /// A generator set over `g` (1..8 points: the second Pedersen generator, a recipient key, the bases of a DLEQ proof): the
    /// id `ed_mul_gens` and `ris_mul_gens_compress` take.  The tables are complete when this returns.  A point that is not on
    /// the curve is refused.  Free the set with `gens_destroy`; the context frees the sets that are left.
    pub fn gens_create(&self, g: &[EdwardsPoint]) -> Result<u64> {
        let fp = flat_ed(g);
        let mut id = 0u64;
        check(unsafe { zc_gens_create(self.ctx, fp.as_ptr(), g.len(), &mut id) })?;
        Ok(id)
    }

    /// Frees the generator set `id` once the work that reads its tables has finished.
    pub fn gens_destroy(&self, id: u64) -> Result<()> {
        check(unsafe { zc_gens_destroy(self.ctx, id) })
    }

    /// `sum_j k[i][j] * G_j` for every row over the set `id` of `count` generators: the same group elements as `&G_j * &k` and
    /// `+` in index order -- equal under `==`, identical encodings, another projective representative.  Not constant-time.
    pub fn ed_mul_gens(&self, id: u64, count: usize, k: &[Vec<Scalar>]) -> Result<Vec<EdwardsPoint>> {
        assert!(k.iter().all(|row| row.len() == count), "one scalar per generator in every row");
        let fk: Vec<u64> = k.iter().flat_map(|row| flat_sc(row)).collect();
        let n = k.len();
        let mut out = vec![0u64; n * 20];
        if n > 0 {
            check(unsafe { zc_ed_mul_gens(self.ctx, id, fk.as_ptr(), out.as_mut_ptr(), n) })?;
        }
        Ok(unflat_ed(&out))
    }

    /// `RistrettoPoint(sum_j k[i][j] * G_j).compress()` for every row: a Pedersen commitment `v * G + r * H` as it goes on the
    /// wire.  The bytes are those of the reference's composition; an identity sum is 32 zero bytes.
    pub fn ris_mul_gens_compress(&self, id: u64, count: usize, k: &[Vec<Scalar>]) -> Result<Vec<CompressedRistretto>> {
        assert!(k.iter().all(|row| row.len() == count), "one scalar per generator in every row");
        let fk: Vec<u64> = k.iter().flat_map(|row| flat_sc(row)).collect();
        let n = k.len();
        let mut out = vec![0u8; n * 32];
        if n > 0 {
            check(unsafe { zc_ris_mul_gens_compress(self.ctx, id, fk.as_ptr(), out.as_mut_ptr(), n) })?;
        }
        Ok(out.chunks_exact(32).map(|b| CompressedRistretto(bytes32(b))).collect())
    }

    /// `p[i][0] + p[i][1] + ...` for every row (`zerocaf_hip_ext_sum_rows.h`): rows of one length, any length -- a tally, an
    /// aggregate of keys or commitments.  The additions are the reference's, associated in the order the header fixes for the
    /// row length (a left fold up to 32 terms; strided slices and a pairwise tree above).  Empty rows give the identity.
    pub fn ed_sum_rows(&self, p: &[Vec<EdwardsPoint>]) -> Result<Vec<EdwardsPoint>> {
        let n = p.len();
        let t = p.first().map_or(0, |row| row.len());
        assert!(p.iter().all(|row| row.len() == t), "rows of one length");
        let mut fp: Vec<u64> = p.iter().flat_map(|row| flat_ed(row)).collect();
        fp.resize(fp.len().max(20), 0);                     // a non-null pointer for rows without terms
        let mut out = vec![0u64; n * 20];
        if n > 0 {
            check(unsafe { zc_ed_sum_rows(self.ctx, fp.as_ptr(), t, out.as_mut_ptr(), n) })?;
        }
        Ok(unflat_ed(&out))
    }

    /// `(sum_j c[i][j].decompress()?).compress()` for every row; `None` where a term does not decode.
    pub fn ris_sum_rows(&self, c: &[Vec<CompressedRistretto>]) -> Result<Vec<Option<CompressedRistretto>>> {
        let n = c.len();
        let t = c.first().map_or(0, |row| row.len());
        assert!(c.iter().all(|row| row.len() == t), "rows of one length");
        let mut flat: Vec<u8> = c.iter().flat_map(|row| row.iter().flat_map(|e| e.0.iter().copied())).collect();
        flat.resize(flat.len().max(32), 0);
        let (mut out, mut ok) = (vec![0u8; n * 32], vec![0u8; n]);
        if n > 0 {
            check(unsafe { zc_ris_sum_rows(self.ctx, flat.as_ptr(), t, out.as_mut_ptr(), ok.as_mut_ptr(), n) })?;
        }
        let enc: Vec<CompressedRistretto> = out.chunks_exact(32).map(|b| CompressedRistretto(bytes32(b))).collect();
        Ok(masked(enc, &ok))
    }
}

// ---- bounded discrete logs (`include/zerocaf_hip_dlog.h`, a header beside `zerocaf_hip.h`): m with P = m * G, 0 <= m < bound
extern "C" {
    /// The baby-step table of the 2^`table_bits` multiples of `point` (of four times it with `ZC_DLOG_COSET4`), on every device of the context.
    pub fn zc_dlog_create(ctx: *mut ZcCtx, point: *const u64, table_bits: u32, flags: u32, id_out: *mut u64) -> c_int;
    /// Frees the table after the context's streams have drained.
    pub fn zc_dlog_destroy(ctx: *mut ZcCtx, id: u64) -> c_int;
    /// `found[i] = 1`, `m_out[i] = m` iff `p[i] == m * G` with `m < bound`; `ok` may be null.
    pub fn zc_ed_dlog(ctx: *mut ZcCtx, id: u64, p: *const u64, bound: u64, m_out: *mut u64, found: *mut u8, ok: *mut u8, n: usize) -> c_int;
    /// The same from Ristretto encodings (a `ZC_DLOG_COSET4` table); `ok[i] = 0` where a row does not decode.
    pub fn zc_ris_dlog(ctx: *mut ZcCtx, id: u64, in32: *const u8, bound: u64, m_out: *mut u64, found: *mut u8, ok: *mut u8, n: usize) -> c_int;
}

/// `flags` of `dlog_create`: the table of 4 G, equality modulo E[4] -- Ristretto equality.
pub const ZC_DLOG_COSET4: u32 = 1;

impl HipBackend {
    /// Builds the baby-step table of `g` with 2^`table_bits` records (`table_bits` = 4..22) and returns the id `ed_dlog` and
    /// `ris_dlog` take.  A point that is not on the curve or lies in E[8] is refused.  Free the table with `dlog_destroy`; the
    /// context frees the tables that are left.
    pub fn dlog_create(&self, g: &EdwardsPoint, table_bits: u32, coset4: bool) -> Result<u64> {
        let fp = flat_ed(std::slice::from_ref(g));
        let mut id = 0u64;
        check(unsafe { zc_dlog_create(self.ctx, fp.as_ptr(), table_bits, if coset4 { ZC_DLOG_COSET4 } else { 0 }, &mut id) })?;
        Ok(id)
    }

    /// Frees the table `id`.
    pub fn dlog_destroy(&self, id: u64) -> Result<()> {
        check(unsafe { zc_dlog_destroy(self.ctx, id) })
    }

    /// For every row the `m < bound` with `p[i] == m * G` (with a coset4 table: `p[i] - m * G` in E[4]), or `None` -- also for a
    /// row that is no point of the curve.  Nothing is constant-time.
    pub fn ed_dlog(&self, id: u64, p: &[EdwardsPoint], bound: u64) -> Result<Vec<Option<u64>>> {
        let fp = flat_ed(p);
        let n = p.len();
        let (mut m, mut found) = (vec![0u64; n], vec![0u8; n]);
        if n > 0 {
            check(unsafe { zc_ed_dlog(self.ctx, id, fp.as_ptr(), bound, m.as_mut_ptr(), found.as_mut_ptr(), std::ptr::null_mut(), n) })?;
        }
        Ok(masked(m, &found))
    }

    /// The same from Ristretto encodings (the table must have been created with `coset4`): `None` where a row does not decode.
    pub fn ris_dlog(&self, id: u64, c: &[CompressedRistretto], bound: u64) -> Result<Vec<Option<u64>>> {
        let flat: Vec<u8> = c.iter().flat_map(|e| e.0.iter().copied()).collect();
        let n = c.len();
        let (mut m, mut found) = (vec![0u64; n], vec![0u8; n]);
        if n > 0 {
            check(unsafe { zc_ris_dlog(self.ctx, id, flat.as_ptr(), bound, m.as_mut_ptr(), found.as_mut_ptr(), std::ptr::null_mut(), n) })?;
        }
        Ok(masked(m, &found))
    }
}

// ---- scalar vector ops (`include/zerocaf_hip_scvec.h`, a header beside `zerocaf_hip.h`): row sums, inner products, power rows mod L
extern "C" {
    /// `out[i] = sum_j a[i][j] mod L`; `a` is `n * terms * 5` limbs, row-major.
    pub fn zc_sc_sum_rows(ctx: *mut ZcCtx, a: *const u64, terms: usize, out: *mut u64, n: usize) -> c_int;
    /// `out[i] = sum_j a[i][j] * b[i][j] mod L`; with `ZC_SC_DOT_SHARED_B`, `b` is one row of `terms * 5` limbs for every row.
    pub fn zc_sc_dot_rows(ctx: *mut ZcCtx, a: *const u64, b: *const u64, terms: usize, flags: u32, out: *mut u64, n: usize) -> c_int;
    /// `out[i][j] = x[i]^j mod L` for `j < terms`; `out[i][0] = 1` also for `x = 0`.
    pub fn zc_sc_powers(ctx: *mut ZcCtx, x: *const u64, terms: usize, out: *mut u64, n: usize) -> c_int;
}

/// `flags` of `zc_sc_dot_rows`: `b` is one row that every row of `a` uses.
pub const ZC_SC_DOT_SHARED_B: u32 = 1;

impl HipBackend {
    /// `a[i][0] + a[i][1] + ...` mod L for every row: rows of one length, any length.  Empty rows give zero.
    pub fn sc_sum_rows(&self, a: &[Vec<Scalar>]) -> Result<Vec<Scalar>> {
        let n = a.len();
        let terms = a.first().map_or(0, |r| r.len());
        assert!(a.iter().all(|r| r.len() == terms), "rows of one length");
        let mut fa: Vec<u64> = a.iter().flat_map(|r| flat_sc(r)).collect();
        fa.resize(fa.len() + 5, 0);
        let mut out = vec![0u64; n * 5];
        if n > 0 {
            check(unsafe { zc_sc_sum_rows(self.ctx, fa.as_ptr(), terms, out.as_mut_ptr(), n) })?;
        }
        Ok(unflat_sc(&out))
    }

    /// `sum_j a[i][j] * b[i][j]` mod L for every row; `a` and `b` have one shape.
    pub fn sc_dot_rows(&self, a: &[Vec<Scalar>], b: &[Vec<Scalar>]) -> Result<Vec<Scalar>> {
        let n = a.len();
        let terms = a.first().map_or(0, |r| r.len());
        assert!(b.len() == n && a.iter().chain(b.iter()).all(|r| r.len() == terms), "a and b of one shape");
        let mut fa: Vec<u64> = a.iter().flat_map(|r| flat_sc(r)).collect();
        let mut fb: Vec<u64> = b.iter().flat_map(|r| flat_sc(r)).collect();
        fa.resize(fa.len() + 5, 0);
        fb.resize(fb.len() + 5, 0);
        let mut out = vec![0u64; n * 5];
        if n > 0 {
            check(unsafe { zc_sc_dot_rows(self.ctx, fa.as_ptr(), fb.as_ptr(), terms, 0, out.as_mut_ptr(), n) })?;
        }
        Ok(unflat_sc(&out))
    }

    /// `sum_j a[i][j] * b[j]` mod L for every row: one row of `b` for all (weights, Lagrange coefficients, `y^n`).
    pub fn sc_dot_rows_shared(&self, a: &[Vec<Scalar>], b: &[Scalar]) -> Result<Vec<Scalar>> {
        let n = a.len();
        let terms = b.len();
        assert!(a.iter().all(|r| r.len() == terms), "every row as long as b");
        let mut fa: Vec<u64> = a.iter().flat_map(|r| flat_sc(r)).collect();
        let mut fb = flat_sc(b);
        fa.resize(fa.len() + 5, 0);
        fb.resize(fb.len() + 5, 0);
        let mut out = vec![0u64; n * 5];
        if n > 0 {
            check(unsafe { zc_sc_dot_rows(self.ctx, fa.as_ptr(), fb.as_ptr(), terms, ZC_SC_DOT_SHARED_B, out.as_mut_ptr(), n) })?;
        }
        Ok(unflat_sc(&out))
    }

    /// `x[i]^0, x[i]^1, ..., x[i]^(terms - 1)` mod L for every `x[i]`; the first is 1 also for `x = 0`.
    pub fn sc_powers(&self, x: &[Scalar], terms: usize) -> Result<Vec<Vec<Scalar>>> {
        let n = x.len();
        let fx = flat_sc(x);
        let mut out = vec![0u64; n * terms * 5];
        if n > 0 && terms > 0 {
            check(unsafe { zc_sc_powers(self.ctx, fx.as_ptr(), terms, out.as_mut_ptr(), n) })?;
        }
        if terms == 0 {
            return Ok(vec![Vec::new(); n]);
        }
        Ok(out.chunks_exact(terms * 5).map(unflat_sc).collect())
    }
}
