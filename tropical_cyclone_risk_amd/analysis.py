"""What the analyses of track files (hazard, landfall, climatology, windfield, loss, rainfall and those built on them) share:
NumPy-or-torch planes, the library context of one call, the group index of the storms, reading (file, year) groups from track
files, and their command lines.  The per-site scan they share on top of this is sitescan.py.

A site analysis's command line is its own options plus five steps, one function each in the CLI section: ``finish_parse`` (what the
options ask of each other, and that sites were given), ``load_inputs`` (sites and track planes as ``Inputs``), ``save_npz`` (the
analysis's arrays and the tail every .npz has), ``print_summary`` (the one line on stdout) and ``print_site_rows`` /
``print_site_tables`` (the per-site tables of up to 10 sites).  hazard, windfield and rainfall differ in the analysis alone:
``threshold_main`` is the body of all three."""
import argparse
import collections
import ctypes as C

import numpy as np

from . import _lib

DEFAULT_THRESHOLDS = np.arange(10, 81, 5).astype(np.float64)
ENV_VARS = ('u250_trks', 'v250_trks', 'u850_trks', 'v850_trks')
# what load_inputs returns: v and env are None without wind, dt_s without spacing; total_years is the number of groups
Inputs = collections.namedtuple('Inputs', 'site_lon site_lat lon lat vmax v env groups gfile gyear dt_s total_years')
SITE_ROW = '  site (%.4f, %.4f)'          # how every per-site line of a command line's tables begins


# ------------------------------------------------------------------------------------------------------------- arrays
def is_tensor(x):
    return type(x).__module__.startswith('torch')


def to_numpy(a):
    return np.asarray(a.cpu() if is_tensor(a) else a)


class Flavour:
    """NumPy arrays, or torch tensors on one device, after a first array: the array module ``xp``, the device ``dev`` (None for
    NumPy), and what an analysis does in either flavour: convert, allocate, make contiguous, take a pointer."""
    _KINDS = {'u1': 'uint8', 'i4': 'int32', 'i8': 'int64', 'f8': 'float64'}

    def __init__(self, first):
        self.torch = is_tensor(first)
        if self.torch:
            import torch
            self.xp, self.dev = torch, first.device
        else:
            self.xp, self.dev = np, None

    def conv(self, a):
        """a as fp64 of this flavour."""
        if self.torch:
            return self.xp.as_tensor(a, dtype=self.xp.float64, device=self.dev)
        return np.asarray(to_numpy(a), dtype=np.float64)

    def new(self, shape, kind):
        """An uninitialised array; kind: 'u1', 'i4', 'i8' or 'f8'."""
        if self.torch:
            return self.xp.empty(shape, dtype=getattr(self.xp, self._KINDS[kind]), device=self.dev)
        return np.empty(shape, dtype=kind)

    def contiguous(self, a):
        return a.contiguous() if self.torch else np.ascontiguousarray(a)

    def ptr(self, a):
        return a.data_ptr() if self.torch else a.ctypes.data

    def context(self, engine, device):
        """The Context of a call on arrays of this flavour (device: the device index of a NumPy call)."""
        return Context(engine, self.dev if self.torch else device)


def as_planes(arrays, names):
    """The track planes as fp64 arrays of the type and on the device of the first: (planes, their Flavour)."""
    fl = Flavour(arrays[0])
    planes = [fl.conv(a) for a in arrays]
    if planes[0].ndim != 2 or any(tuple(p.shape) != tuple(planes[0].shape) for p in planes):
        raise ValueError('%s must be [n_trk][n_t] arrays of one shape' % names)
    return planes, fl


# ------------------------------------------------------------------------------------------------------------ context
class Context:
    """The caller's engine (anything with a library handle `.h`), or a context of our own for one ``with`` block.  device: the
    device index (the NumPy flavour: `call` runs the ``_host`` entry points), or the torch device of the inputs (`call` runs the
    ``_dev`` entry points on its current stream)."""

    def __init__(self, engine, device):
        self.L = _lib.lib()
        self.dev = None if isinstance(device, (int, np.integer)) else device
        if self.dev is not None:
            import torch
            self._stream = lambda: torch.cuda.current_stream(self.dev)
            device = self.dev.index if self.dev.index is not None else torch.cuda.current_device()
        self.own = engine is None
        if self.own:
            h = C.c_void_p()
            if self.L.tcr_ctx_create(int(device), C.byref(h)) != 0:
                raise _lib.TcrError(self.L.tcr_last_error(None).decode())
            self.h = h
        else:
            self.h = engine.h

    def check(self, rc):
        if rc != 0:
            raise _lib.TcrError(self.L.tcr_last_error(self.h).decode())

    def call(self, entry, *args):
        if self.dev is not None:
            self.check(getattr(self.L, entry + '_dev')(self.h, *args, C.c_void_p(self._stream().cuda_stream)))
        else:
            self.check(getattr(self.L, entry + '_host')(self.h, *args))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        if self.own and self.h:
            if self.dev is not None:
                self._stream().synchronize()                    # the context's workspaces go with it
            self.L.tcr_ctx_destroy(self.h)
            self.h = None


# ------------------------------------------------------------------------------------------------------------- groups
def group_index(groups, n_trk, n_groups=None, bad='groups must hold one non-negative integer per storm',
                over='a group index is >= n_groups'):
    """(int64 group of every storm, n_groups): one non-negative integer per storm, n_groups by default max + 1 (1 without
    storms), every index < n_groups.  bad, over: the caller's ValueError texts."""
    g = to_numpy(groups).reshape(-1)
    if g.shape[0] != n_trk or (n_trk and (g.dtype.kind not in 'iu' or g.min() < 0)):
        raise ValueError(bad)
    g = g.astype(np.int64)
    n_groups = int(n_groups if n_groups is not None else (g.max() + 1 if n_trk else 1))
    if n_trk and g.max() >= n_groups:
        raise ValueError(over)
    return g, n_groups


# -------------------------------------------------------------------------------------------------------- track files
def load_groups(files, extra=()):
    """Read the track files and number their (file, year) groups: every year of every file's `year` coordinate is one group,
    years without storms included.  Returns lon, lat, vmax [n_trk][n_t], the group of every storm, group_file and group_year
    [n_group] (the group -> (file index, year) map).  extra: names of further variables of the files; when given, a seventh
    element {name: [one array per file]} follows."""
    from . import io as tio
    lon, lat, vmax, groups, gfile, gyear = [], [], [], [], [], []
    more = {name: [] for name in extra}
    for k, fn in enumerate(files):
        d = tio.read_tracks(fn)
        for name in extra:
            more[name].append(np.asarray(d[name]))
        years = np.asarray(d['year']).astype(np.int64).reshape(-1)
        tc_years = np.asarray(d['tc_years']).astype(np.int64).reshape(-1)
        pos = {int(y): i for i, y in enumerate(years)}
        if not set(int(y) for y in tc_years) <= set(pos):
            raise ValueError('%s: a storm year is not in the file\'s year coordinate' % fn)
        groups.append(len(gfile) + np.array([pos[int(y)] for y in tc_years], dtype=np.int64))
        gfile += [k] * len(years)
        gyear += list(years)
        for dst, key in ((lon, 'lon_trks'), (lat, 'lat_trks'), (vmax, 'vmax_trks')):
            dst.append(np.asarray(d[key], dtype=np.float64))
    n_t = {a.shape[1] for a in lon}
    if len(n_t) != 1:
        raise ValueError('the track files have different time axes: %s' % sorted(n_t))
    res = (np.concatenate(lon), np.concatenate(lat), np.concatenate(vmax), np.concatenate(groups),
           np.array(gfile, dtype=np.int64), np.array(gyear, dtype=np.int64))
    return res + (more,) if extra else res


def sample_spacing(times):
    """dt (s) of the track files' `time` axes (one array per file): time[1] - time[0], uniform to a relative 1e-9 and equal in
    every file; a file of one sample takes the namelist's output interval."""
    from . import namelist
    dts = []
    for t in times:
        t = np.asarray(t, dtype=np.float64).reshape(-1)
        if t.size < 2:
            dts.append(float(namelist.output_interval_s))
            continue
        dt = float(t[1] - t[0])
        if not dt > 0 or np.any(np.abs(np.diff(t) - dt) > 1e-9 * dt):
            raise ValueError('the time axis of a track file is not uniform')
        dts.append(dt)
    if any(abs(d - dts[0]) > 1e-9 * dts[0] for d in dts):
        raise ValueError('the track files have different sample spacings: %s' % sorted(set(dts)))
    return dts[0]


def load_wind_planes(files):
    """What the wind footprint reads from track files: lon, lat, vmax, v [n_trk][n_t], env (the four ENV_VARS planes), the
    groups, group_file and group_year of load_groups, and the sample spacing dt (s)."""
    lon, lat, vmax, groups, gfile, gyear, more = load_groups(files, extra=('v_trks',) + ENV_VARS + ('time',))
    v, *env = (np.concatenate([np.asarray(a, dtype=np.float64) for a in more[k]]) for k in ('v_trks',) + ENV_VARS)
    return lon, lat, vmax, v, env, groups, gfile, gyear, sample_spacing(more['time'])


def group_meta(files, gfile, gyear):
    """The group -> (file, year) map as every analysis saves it: the tail of its np.savez."""
    return dict(group_file=gfile, group_year=gyear, files=np.array([str(f) for f in files]))


# ---------------------------------------------------------------------------------------------------------------- CLI
def parse_range(text, what):
    """LO:HI:STEP, both ends included."""
    try:
        lo, hi, step = (float(x) for x in text.split(':'))
    except ValueError:
        raise argparse.ArgumentTypeError('%s: expected LO:HI:STEP, got %r' % (what, text))
    if not step > 0 or hi < lo:
        raise argparse.ArgumentTypeError('%s: need STEP > 0 and HI >= LO, got %r' % (what, text))
    return lo + step * np.arange(int(np.floor((hi - lo) / step + 1e-9)) + 1)


def parse_site(text):
    try:
        lon, lat = (float(x) for x in text.split(','))
    except ValueError:
        raise argparse.ArgumentTypeError('--site: expected LON,LAT, got %r' % text)
    return lon, lat


def parse_grid(text):
    parts = text.split(',')
    if len(parts) != 2:
        raise argparse.ArgumentTypeError('--grid: expected LON0:LON1:DLON,LAT0:LAT1:DLAT, got %r' % text)
    return parse_range(parts[0], '--grid lon'), parse_range(parts[1], '--grid lat')


def parse_periods(text):
    try:
        T = [float(x) for x in text.split(',')]
    except ValueError:
        raise argparse.ArgumentTypeError('--return-periods: expected T1,T2,..., got %r' % text)
    if not T or not all(np.isfinite(t) and t > 0 for t in T):
        raise argparse.ArgumentTypeError('--return-periods: need finite values > 0, got %r' % text)
    return np.array(T)


def parse_exceedances(text):
    try:
        k = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError('--tail-exceedances: expected an integer, got %r' % text)
    if not 2 <= k <= _lib.TAIL_MAX_K:
        raise argparse.ArgumentTypeError('--tail-exceedances: need 2 <= K <= %d, got %r' % (_lib.TAIL_MAX_K, text))
    return k


def add_track_args(p, out_default):
    p.add_argument('tracks', nargs='+', help='track files (ensemble members); every year of every file is one group')
    p.add_argument('--out', default=out_default)
    p.add_argument('--device', type=int, default=0)


def add_site_args(p):
    p.add_argument('--site', type=parse_site, action='append', default=[], metavar='LON,LAT',
                   help='repeatable; write --site=LON,LAT when LON is negative')
    p.add_argument('--sites', metavar='FILE.csv', help='one LON,LAT per line (lines that are not two numbers are skipped)')
    p.add_argument('--grid', type=parse_grid, metavar='LON0:LON1:DLON,LAT0:LAT1:DLAT')


def add_footprint_args(p):
    p.add_argument('--rmax-km', type=float, default=None, help='constant radius of maximum wind (default: Willoughby et al. 2006)')
    p.add_argument('--r-out-km', type=float, default=500.0)
    p.add_argument('--substeps', type=int, default=1, help='evaluation points per sample interval (1 = the samples only)')
    p.add_argument('--ck-cd', type=float, default=None, help='Ck / Cd of the profile (default: the namelist\'s)')


def add_threshold_arg(p):
    p.add_argument('--thresholds', type=lambda t: parse_range(t, '--thresholds'), default=DEFAULT_THRESHOLDS, metavar='LO:HI:STEP')


def add_return_period_arg(p, what):
    p.add_argument('--return-periods', type=parse_periods, default=None, metavar='T1,T2,...',
                   help='also write return_level, the %s of these return periods (years) at every site, and n_reach '
                        '(levels.site_return_levels)' % what)
    p.add_argument('--tail-exceedances', type=parse_exceedances, default=None, metavar='K',
                   help='with --return-periods: also write tail_level, the levels from a generalized Pareto tail fitted to the K '
                        'largest storms of every site (levels.row_tail: return periods past the record), tail_xi, tail_sigma and '
                        'tail_threshold')


def parse_floor(text):
    try:
        v = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError('--events-min: expected a number, got %r' % text)
    if v != v:
        raise argparse.ArgumentTypeError('--events-min: the floor must not be NaN')
    return v


def add_events_arg(p, what):
    p.add_argument('--events-out', default=None, metavar='FILE.npz',
                   help='also write the event table: per site, the storms whose %s is at or above --events-min, with that value '
                        '(events.site_event_table; a pass of its own)' % what)
    p.add_argument('--events-min', type=parse_floor, default=None, metavar='V', help='the floor of --events-out (required with it)')


def read_sites_csv(fn):
    out = []
    for line in open(fn):
        f = line.replace(';', ',').split(',')
        try:
            if len(f) >= 2:
                out.append((float(f[0]), float(f[1])))
        except ValueError:
            pass
    return out


def collect_sites(args):
    """The sites of --site, --sites and --grid, in that order: (lon [n], lat [n])."""
    pts = list(args.site)
    if args.sites:
        pts += read_sites_csv(args.sites)
    lon = [p[0] for p in pts]
    lat = [p[1] for p in pts]
    if args.grid is not None:
        glon, glat = np.meshgrid(args.grid[0], args.grid[1])
        lon += list(glon.ravel())
        lat += list(glat.ravel())
    return np.array(lon, dtype=np.float64), np.array(lat, dtype=np.float64)


def finish_parse(p, a, no_tail=None):
    """What a site analysis's options ask of each other after parsing, in one order: those of add_return_period_arg (no_tail: the
    analysis's sentence when it does not offer --tail-exceedances) and of add_events_arg where the parser has them, and that
    sites were given.  Returns a."""
    if getattr(a, 'tail_exceedances', None) is not None and (no_tail is not None or a.return_periods is None):
        p.error(no_tail or '--tail-exceedances needs --return-periods')
    if getattr(a, 'events_out', None) is not None and a.events_min is None:
        p.error('--events-out needs --events-min')
    if getattr(a, 'events_min', None) is not None and a.events_out is None:
        p.error('--events-min needs --events-out')
    if not (a.site or a.sites or a.grid):
        p.error('give sites with --site, --sites or --grid')
    return a


def load_inputs(args, wind=False, spacing=True, sites=None):
    """The parsed command line's inputs: the sites (sites: the caller's own (lon, lat); None: those of collect_sites, and
    SystemExit without any), then the track files' planes through load_wind_planes (wind) or load_groups, with their sample
    spacing where asked for."""
    site_lon, site_lat = collect_sites(args) if sites is None else sites
    if site_lon.size == 0:
        raise SystemExit('no sites')
    v = env = dt = None
    if wind:
        lon, lat, vmax, v, env, groups, gfile, gyear, dt = load_wind_planes(args.tracks)
    elif spacing:
        lon, lat, vmax, groups, gfile, gyear, more = load_groups(args.tracks, extra=('time',))
        dt = sample_spacing(more['time'])
    else:
        lon, lat, vmax, groups, gfile, gyear = load_groups(args.tracks)
    return Inputs(site_lon, site_lat, lon, lat, vmax, v, env, groups, gfile, gyear, dt, len(gfile))


def save_npz(args, inp, arrays, recorded=(), more=()):
    """Write args.out: the analysis's own arrays, then what every analysis saves (the sites, total_years, dt_s where the files'
    spacing was read, group_meta) and the options among recorded ('r_out_km', 'substeps', 'rmax_km': NaN for None) as the command
    line had them; more: the keys --return-periods adds."""
    tail = dict(site_lon=inp.site_lon, site_lat=inp.site_lat, total_years=inp.total_years)
    for name in recorded:
        value = getattr(args, name)
        tail[name] = np.nan if value is None else value
    if inp.dt_s is not None:
        tail['dt_s'] = inp.dt_s
    np.savez(args.out, **arrays, **tail, **group_meta(args.tracks, inp.gfile, inp.gyear), **dict(more))


def print_summary(args, inp, middle='', site_note=''):
    """The line every command line prints after writing its .npz; middle: the analysis's own part, with its leading comma."""
    print('%d sites%s, %d storms, %d groups (%d files), total_years = %d%s -> %s'
          % (inp.site_lon.size, site_note, inp.lon.shape[0], inp.total_years, len(args.tracks), inp.total_years, middle, args.out))


def print_site_rows(header, site_lon, site_lat, rows, fmt=None):
    """One line per site under a header (None: none): the [n_site][k] numbers of rows, each through fmt, or with fmt None the
    ready texts of rows."""
    if header is not None:
        print(header)
    for i in range(site_lon.size):
        print(SITE_ROW % (site_lon[i], site_lat[i]) + ': ' + (rows[i] if fmt is None else ' '.join(fmt % v for v in rows[i])))


def print_site_tables(header, site_lon, site_lat, labels, tables, fmt):
    """One small table per site under a header: the site's line, then a row of tables[site] per label."""
    print(header)
    for i in range(site_lon.size):
        print(SITE_ROW % (site_lon[i], site_lat[i]))
        for label, row in zip(labels, tables[i]):
            print('    ' + label + ' '.join(fmt % x for x in row))


def print_return_periods(thresholds, site_lon, site_lat, rp, unit='m/s'):
    """The return-period table of up to 10 sites (more: nothing).  unit: of the thresholds."""
    if site_lon.size <= 10:
        print_site_rows('return period (years) by threshold (%s): ' % unit + ' '.join('%6g' % t for t in thresholds), site_lon,
                        site_lat, rp, '%6.3g')


def threshold_main(args, inp, block, tracks, key, unit='m/s', arrays=(), recorded=(), middle=''):
    """What the command lines of hazard, windfield and rainfall do with their inputs, which is the same but for the analysis:
    block(tracks, lon_block, lat_block, plane=False, device=0) is the analysis on some sites, with its per-storm plane (key, in
    unit) when asked.  One plain call, or with --return-periods the blocked pass of levels.device_levels; the .npz (arrays: the
    analysis's further keys), the summary line (middle), the tables, and with --events-out a pass of its own through the same block."""
    from . import events, hazard, levels
    with_plane = lambda t, x, y: block(t, x, y, plane=True)                                 # noqa: E731
    more = {}
    if args.return_periods is None:
        res = block(tracks, inp.site_lon, inp.site_lat, device=args.device)
    else:
        res = levels.device_levels(with_plane, tracks, inp.site_lon, inp.site_lat, inp.total_years, args.return_periods, key,
                                   args.device, tail_exceedances=args.tail_exceedances)
        more = levels.npz_keys(res)
    rp = hazard.return_periods(res['counts'], inp.total_years)
    save_npz(args, inp, dict(counts=res['counts'], return_period=rp, thresholds=res['thresholds'], **dict(arrays)), recorded, more)
    print_summary(args, inp, middle)
    print_return_periods(res['thresholds'], inp.site_lon, inp.site_lat, rp, unit=unit)
    if more:
        levels.print_return_levels(res, inp.site_lon, inp.site_lat, unit=unit)
    if args.events_out is not None:
        events.write_cli_events(args, with_plane, tracks, inp.site_lon, inp.site_lat, key, unit, inp.groups, inp.gfile, inp.gyear)
    return 0
