"""Generate the beta/corr gap fixture from the REAL reference (carkod/binquant).

    python tests/golden/make_golden_beta_gaps.py     # writes beta_corr_gaps.npz

Runs where the reference is mounted only; the shim directory and the
child-process scheme are make_golden.py's (imported, not copied). Only
numeric inputs and outputs are written.

ContextEvaluator.dynamic_btc_beta_corr (producers/context_evaluator.py:154-194,
window 50) on every prefix of index-aligned (symbol, BTC) closes with missing
(NaN) and zero candles, exactly as make_golden.py section 6 calls it:
round_numbers is the shim's identity, so the values are unrounded, and the
method's own NaN -> 0 mapping is in them.

  gap_alt       symbol NaN at 200, at 300-302 and at the last candle
  late_listing  symbol NaN on [0, 120)
  long_gap      symbol NaN on 150-219 (longer than the window)
  gap_btc       BTC NaN at 180-181, symbol NaN at 181 and at 250
  zero_close    symbol close 0.0 at 260 (returns -inf, then +inf)
  flat_gap      symbol flat on 200-260 with a NaN at 230 (pandas' same-value
                rule across a gap: exact 0 covariance, NaN correlation)
  sparse        n = 120, symbol NaN at every third candle: never 50 valid
                pairs, (0, 0) throughout

Per case: <case>__close, <case>__btc, <case>__beta_last, <case>__corr_last
(index 0 NaN: the method needs two candles).
"""

from __future__ import annotations

import os
import subprocess
import sys
import tempfile
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import make_golden as mg   # noqa: E402  (shim writer + reference location)

WINDOW = 50
CASES = {   # name: (n, seed, rho)
    "gap_alt": (420, 71, 0.7),
    "late_listing": (400, 73, 0.5),
    "long_gap": (420, 75, -0.4),
    "gap_btc": (400, 77, 0.6),
    "zero_close": (420, 79, 0.7),
    "flat_gap": (400, 81, 0.5),
    "sparse": (120, 83, 0.6),
}


def build_case(name: str):
    import numpy as np

    n, seed, rho = CASES[name]
    rb = np.random.default_rng(seed).normal(0, 0.004, n)
    ra = rho * rb + np.sqrt(1 - rho**2) * np.random.default_rng(seed + 1).normal(0, 0.006, n)
    btc = 60000.0 * np.exp(np.cumsum(rb))
    alt = 3.0 * np.exp(np.cumsum(ra))
    if name == "gap_alt":
        alt[[200, 300, 301, 302, n - 1]] = np.nan
    elif name == "late_listing":
        alt[:120] = np.nan
    elif name == "long_gap":
        alt[150:220] = np.nan
    elif name == "gap_btc":
        btc[180:182] = np.nan
        alt[[181, 250]] = np.nan
    elif name == "zero_close":
        alt[260] = 0.0
    elif name == "flat_gap":
        alt[200:261] = alt[200]
        alt[230] = np.nan
    elif name == "sparse":
        alt[::3] = np.nan
    return alt, btc


def child(out_dir: Path) -> None:
    import warnings
    from types import SimpleNamespace

    import numpy as np
    import pandas as pd

    from producers.context_evaluator import ContextEvaluator

    out = {}
    for name, (n, _, _) in CASES.items():
        alt, btc = build_case(name)
        betas, corrs = [], []
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)   # log(0), inf - inf inside the reference
            for m in range(2, n + 1):
                ns = SimpleNamespace(df_15m=pd.DataFrame({"close": alt[:m]}),
                                     df_btc_15m=pd.DataFrame({"close": btc[:m]}))
                b, c = ContextEvaluator.dynamic_btc_beta_corr(ns, window=WINDOW)
                betas.append(b)
                corrs.append(c)
        out[f"{name}__close"] = alt
        out[f"{name}__btc"] = btc
        out[f"{name}__beta_last"] = np.array([np.nan] + betas, dtype=np.float64)
        out[f"{name}__corr_last"] = np.array([np.nan] + corrs, dtype=np.float64)
        nz = int(np.count_nonzero(out[f"{name}__beta_last"][1:]))
        print(f"{name}: n={n}, NaN closes {int(np.isnan(alt).sum())} / {int(np.isnan(btc).sum())}, "
              f"{nz} non-zero betas")
    np.savez_compressed(out_dir / "beta_corr_gaps.npz", **out)


def main() -> None:
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(Path(sys.argv[2]))
        return
    if not mg.REFERENCE.exists():
        sys.exit("make_golden_beta_gaps.py runs only where the reference is mounted")
    with tempfile.TemporaryDirectory(prefix="bq_shim_") as tmp:
        shim = Path(tmp)
        mg.write_shim(shim)
        env = dict(os.environ)
        env["PYTHONPATH"] = f"{shim}:{mg.REFERENCE}"
        env["PYTHONDONTWRITEBYTECODE"] = "1"
        env["ENV"] = "ci"
        subprocess.run([sys.executable, __file__, "--child", str(HERE)], check=True, env=env, cwd=tmp)


if __name__ == "__main__":
    main()
