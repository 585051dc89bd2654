"""Golden vectors for the PI / chi / RH preprocessing at ERA5's own 37 pressure levels and on axes of two, three and four
levels, made by importing the reference.

Runs the reference's own `thermo.CAPE_PI_vectorized`, `thermo.sat_deficit` and `thermo.conv_q_to_rh` (thermo/thermo.py)
on the column family of tests/thermo_columns.py, which reaches the branches that tests/golden/thermo_cases.npz does not
(parcel saturated at the lowest level, last hit at the top level, levels above the entropy table, non-uniform levels).
Only runs where /root/reference exists:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_thermo_era5.py

Writes thermo_cases_era5.npz; thermo_cases.npz and entropy_table.npz stay as make_golden_thermo.py left them.
"""
import os
import sys

import numpy as np
import scipy

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from ref_harness import REF, import_reference  # noqa: E402
from tests import thermo_columns as tc  # noqa: E402

SEED = 20261019
N_ERA5, N_FEW = 384, 64


def main():
    ref = import_reference()
    from thermo import thermo
    nl = ref.namelist
    assert nl.select_thermo == 1 and nl.select_interp == 2
    nl.src_directory = REF                     # where CAPE_PI_vectorized looks for the table
    rng = np.random.default_rng(SEED)
    sets = {'era5': (tc.ERA5_LEVELS_PA,) + tc.family(rng, N_ERA5, tc.ERA5_LEVELS_PA)}
    sets.update(tc.few_levels(rng, N_FEW))
    out = {}
    for tag, (p, sst, psl, T, r) in sets.items():
        # the reference indexes [level, lat, lon]: the columns go in as one row of latitude
        with np.errstate(all='ignore'):
            pi = thermo.CAPE_PI_vectorized(sst[None], psl[None], p, T[:, None], r[:, None])[0]
            k_mid = int(np.argmin(np.abs(p - nl.p_midlevel)))
            chi = thermo.sat_deficit(sst, psl, T[k_mid], float(p[k_mid]), r[k_mid])
            rhm = thermo.conv_q_to_rh(T[k_mid], r[k_mid], float(p[k_mid]))
        out.update({tag + '_p': p, tag + '_sst': sst, tag + '_psl': psl, tag + '_T': T, tag + '_r': r,
                    tag + '_PI': pi, tag + '_chi': chi, tag + '_rh_mid': rhm, tag + '_k_mid': np.int64(k_mid)})
        print(tag, 'PI range', np.nanmin(pi), np.nanmax(pi), 'zeros', int((pi == 0).sum()), 'of', pi.size)
    out['versions'] = np.array(['numpy ' + np.__version__, 'scipy ' + scipy.__version__])
    out['Ck_over_Cd'] = np.float64(nl.Ck / nl.Cd)
    out['p_midlevel'] = np.float64(nl.p_midlevel)
    fn = os.path.join(HERE, 'thermo_cases_era5.npz')
    np.savez_compressed(fn, **out)
    print('wrote thermo_cases_era5.npz, %d bytes' % os.path.getsize(fn))


if __name__ == '__main__':
    main()
