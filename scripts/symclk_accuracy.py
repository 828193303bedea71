"""How well vdl2gpu_symclk_t's definition measures a transmitter (CPU only, no GPU): the float64 restatement (tests/symclk_ref.py) on
the CPU model's 84 kS/s plane against the synthetic transmitter's truth, the cases tests/test_symclk_model.py holds -- cs16 at 2 and
10 MS/s and cu8 at 2 MS/s, eight bursts each from about 120 to about 4550 symbols at a random fraction of a symbol, noise 1.7, the
symbol clock 0, +50 and -30 ppm off.  Prints the table and the bounds the GPU tests take from it (twice the worst error).

    python scripts/symclk_accuracy.py > profiles/r24_symclk_accuracy.txt
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import __graft_entry__ as g  # noqa: E402


def main():
    g.build()
    import levels_ref as LR
    import symclk_ref as R
    from oracle import oracle as O
    rows = R.accuracy_table(O)
    print("# vdl2gpu_symclk_t (VDL2GPU_F_SYMCLK): the definition's accuracy against the synthetic transmitter, float64 on the CPU model's plane")
    print("# (scripts/symclk_accuracy.py; tests/test_symclk_model.py holds these numbers).  toa error: toa_sample minus the true centre of the")
    print("# first symbol behind the unique word, (Burst.t0 + 21 T) * sdrinrate; clock error: clock_ppm minus Burst.sym_ppm.")
    print("# D = %.6f (the centroid of the sub-phase-0 taps: derived, not fitted)" % R.centroid_delay(LR.mflt_taps()))
    print("# fmt  sdrinrate  info  nsym nseg  sym_ppm  toa_error_us  clock_ppm  clock_error  tau_rms")
    for r in rows:
        print("%-4s %9d  %4d  %4d  %2d    %+4.0f     %+8.4f   %+8.3f     %+7.3f   %.4f"
              % (r["fmt"], r["rate"], r["info"], r["nsym"], r["nseg"], r["sym_ppm"], r["toa_err_us"], r["ppm"], r["ppm_err"], r["tau_rms"]))
    toa, ppm_long, ppm_mid, toa_mean = R.worst(rows)
    print("#")
    print("# toa_sample: worst |error| %.4f us over all %d bursts; mean %+.4f us -- NOT small against the scatter:" % (toa, len(rows), toa_mean))
    for f in R.FORMATS:
        a = np.array([r["toa_err_us"] for r in rows if (r["fmt"], r["rate"]) == f[:2]])
        print("#   %-4s %9d: mean %+.4f us, standard deviation %.4f us, %+.4f .. %+.4f us" % (f[0], f[1], a.mean(), a.std(), a.min(), a.max()))
    print("#   (an offset of a sixtieth of an 84 kS/s sample with the derived D; reported, not absorbed: the bound is on the error itself)")
    print("# clock_ppm: worst |error| %.3f ppm with nseg >= 10, %.3f ppm with 3 <= nseg < 10; with nseg == 2 the line goes through its" % (ppm_long, ppm_mid))
    print("#   two points (tau_rms 0) and the error reaches %.1f ppm: no bound there; nseg == 1 has no clock_ppm (NaN)"
          % max(abs(r["ppm_err"]) for r in rows if r["nseg"] == 2))
    print("# bounds of tests/test_gpu_symclk.py (twice the worst; the factor is for other seeds): |toa error| <= %.4f us; |clock error| <= %.3f ppm"
          % (2 * toa, 2 * ppm_long))
    print("#   (nseg >= 10), <= %.3f ppm (3 <= nseg < 10)" % (2 * ppm_mid))


if __name__ == "__main__":
    main()
