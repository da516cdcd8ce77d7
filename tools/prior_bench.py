"""What incremental training adds to a partition on the device (csrc/re_prior.hip): gdmix_re_prior_apply + gdmix_re_prior_restore on a
C2-sized synthetic batch (1 M entities x 16 samples x 4 non-zeros), next to the same batch's pack and solve.

    PYTHONPATH=. python tools/prior_bench.py [entities] [steps] > profiles/prior_transform.txt

Device events on the stream around each call, one warm-up, the median of `steps` (with [min, max]). A report, not a bar.
Bytes are the algorithm's: the CSR pass reads value and column (8 B) and writes the value (4 B) per non-zero, reads row_ptr and offset and
writes offset' (12 B) per sample; the CSC pass reads and writes the value (8 B) per non-zero; the gathers of mu and s (16 B per non-zero
in the CSR pass, 8 B in the CSC pass) come from arrays of 16 B per coefficient that fit the L2 / Infinity Cache and are counted once;
the restore reads mu, s, phi, var' and writes theta, theta_thr, variance (56 B per coefficient).
"""
import statistics
import sys

import numpy as np

from gdmix_amd import synthetic

E = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 7
HBM_PEAK = 8.0e12       # bytes/s, MI355X


def timed(torch, fn, steps=STEPS):
    """One warm-up, then `steps` calls, each between two events on the current stream -> (median, min, max) ms, last result."""
    out = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return (statistics.median(ms), min(ms), max(ms)), out


def fmt(t):
    return f"{t[0]:9.3f} ms [{t[1]:.3f}, {t[2]:.3f}]"


def main():
    import torch
    from gdmix_amd.solver import REDeviceSolver, SolverOptions, VAR_SIMPLE
    s = REDeviceSolver(0)
    b = synthetic.make_batch(E, 16, 4, 1024, seed=synthetic.C2_SEED, with_uid=False)
    raw = s.upload(b)
    t_pack, packed = timed(torch, lambda: s.pack(raw))
    P = packed.P
    rng = np.random.default_rng(1)
    mean = 0.3 * rng.standard_normal(P)
    var = np.exp(rng.uniform(np.log(1e-4), np.log(10.0), P))
    none = rng.random(P) < 1.0 / 3.0
    mean[none], var[none] = 0.0, 1.0
    scale = np.sqrt(var)
    scale[packed.coef_ptr_host()[:-1]] = 1.0
    mean_d, scale_d = torch.from_numpy(mean).to(s.device), torch.from_numpy(scale).to(s.device)
    opts = SolverOptions(variance_mode=VAR_SIMPLE)
    t_apply, work = timed(torch, lambda: s.prior_apply(packed, mean_d, scale_d))
    t_solve, solved = timed(torch, lambda: s.solve(work, opts))
    t_plain, _ = timed(torch, lambda: s.solve(packed, opts))
    t_restore, back = timed(torch, lambda: s.prior_restore(packed, mean_d, scale_d, solved.theta, solved.variance))
    apply_bytes = 12.0 * packed.Z + 12.0 * packed.N + 8.0 * packed.Z + 16.0 * P
    restore_bytes = 56.0 * P
    print(f"C2-shaped batch: {packed.E} entities, {packed.N} samples, {packed.Z} non-zeros, {P} coefficients; a third of the priors defaulted; {STEPS} steps")
    print(f"  gdmix_re_pack                                  {fmt(t_pack)}")
    print(f"  gdmix_re_solve, the batch as packed            {fmt(t_plain)}")
    print(f"  gdmix_re_solve, the transformed batch          {fmt(t_solve)}   (another problem: its own iteration counts)")
    for what, t, nbytes in (("gdmix_re_prior_apply (CSR pass + CSC pass)", t_apply, apply_bytes), ("gdmix_re_prior_restore", t_restore, restore_bytes)):
        print(f"  {what:<46s} {fmt(t)}   {nbytes / 1e6:.0f} MB needed, {nbytes / t[0] / 1e6:.0f} GB/s, {100.0 * nbytes / (t[0] * 1e-3) / HBM_PEAK:.1f} % of the HBM peak")
    both = t_apply[0] + t_restore[0]
    print(f"  apply + restore = {both:.3f} ms = {100.0 * both / (t_pack[0] + t_plain[0]):.1f} % of pack + solve ({t_pack[0] + t_plain[0]:.3f} ms), "
          f"{(apply_bytes + restore_bytes) / packed.Z:.1f} B per non-zero")
    # the thing measured is the thing specified: x' of the first rows against the host statement
    z = min(packed.Z, 1 << 16)
    cp = packed.coef_ptr_host()
    ent = np.repeat(np.arange(packed.E), np.diff(packed.ent_nnz_ptr().cpu().numpy()))[:z]
    slot = cp[:-1][ent] + 1 + packed.csr_col()[:z].cpu().numpy()
    want = (packed.csr_val()[:z].cpu().numpy().astype(np.float64) * scale[slot]).astype(np.float32)
    assert np.array_equal(work.csr_val()[:z].cpu().numpy().view(np.uint32), want.view(np.uint32))
    s.close()


if __name__ == "__main__":
    main()
