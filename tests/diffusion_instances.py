"""The kernel instantiations the three diffusion launchers can name, and one value case for each (no GPU needed to import).

launch_error_diffusion (csrc/ediff.hip), launch_variable_diffusion and launch_variance_gate (csrc/vardiff.hip) choose a kernel,
its template arguments and a schedule from the palette, the frame shape, the batch and the device's CU count.  The experiments
library names that choice on stderr (DP_ED_TRACE=1: trace_diffusion in csrc/dp_internal.h, trace_gate in vardiff.hip).  Here:

  NAMED       every instantiation the launchers spell, as tuples (the launchers' own constants restated below)
  SCHEDULES   the launch shapes of the wavefront kernels, per arithmetic family
  CASES       one row per value case of tests/test_gpu_diffusion_instances.py: entry point, palette, (n, h, w), content, parameters,
              switches, and `expect` = (instance, schedule) the row is MEANT to reach, with the launcher condition it is derived from
  UNREACHED   instance -> the launcher condition that rules it out for every palette

tests/test_diffusion_instances_cpu.py checks the table against itself and the boundary widths against the launchers' LDS
expressions restated here; the GPU module asserts the traced instance of every row and that the rows reach NAMED - UNREACHED."""
import collections
import os
import re

import numpy as np

# ---- the launchers' constants (host_logic.h, ediff.hip, vardiff.hip)
QS, QL = 64, 256            # kQueueSmall, kQueueLarge: the traversal queue of the CAP template argument
MAX_TAPS = 16               # kMaxTaps: the generic tap-count instance
MAX_WAVES, NB_WAVES, V_WAVES = 16, 8, 12   # kMaxWaves, kNbWaves (numba arithmetic), kVWaves (variable diffusers)
LDS_LIMIT = 158 * 1024      # what the row-serial kernels may use, with 512 bytes kept back
WIDE_ROW = 60000            # rows from here on leave the wavefront kernels
GATE_MAX_R = 4              # kGateMaxR: the fused gate kernel's largest window radius
_NAMES = {"kQueueSmall": QS, "kQueueLarge": QL, "kMaxTaps": MAX_TAPS, "kMaxWaves": MAX_WAVES, "kNbWaves": NB_WAVES, "true": True, "false": False}

# ---- NAMED
# ed_wavefront_kernel<CAP, NT, EXACT, MAXW, NB, PALS>, python arithmetic: the queue / search kind (DP_EDN), the tap count (the switch
# over ntaps), four or sixteen waves (DP_EDW)
SEARCH_KINDS = {"wide": (QL, 0),      # n_inner > 64 or more than 256 colours: the wide lists
                "coarse": (QS, 1),    # at most 16 colours: the coarse 16^3 lists
                "lists": (QS, 2)}     # 17 .. 256 colours
TAP_INSTANCES = [(3, True), (4, True), (6, True), (7, True), (10, True), (12, True), (MAX_TAPS, False)]


def ed_wavefront(kind, ntaps, waves):
    cap, pals = SEARCH_KINDS[kind]
    nt, exact = (ntaps, True) if (ntaps, True) in TAP_INSTANCES else (MAX_TAPS, False)
    return ("ed_wavefront", cap, nt, exact, waves, False, pals)


ED_WAVEFRONT_NUMBA = [("ed_wavefront", QS, MAX_TAPS, False, 4, True, 0), ("ed_wavefront", QS, MAX_TAPS, False, NB_WAVES, True, 0)]
NAMED = set()
NAMED |= {("ed_wavefront", cap, nt, exact, waves, False, pals) for cap, pals in SEARCH_KINDS.values() for nt, exact in TAP_INSTANCES
          for waves in (4, MAX_WAVES)}                                                                   # 42
NAMED |= set(ED_WAVEFRONT_NUMBA)                                                                         # 2
NAMED |= {("ed_rowserial", cap, m) for cap in (QS, QL) for m in (1, 4, 16)}                              # 6
NAMED |= {("ed_serial", QS, False), ("ed_serial", QL, False), ("ed_serial", QS, True)}                   # 3
NAMED |= {("var_wavefront", cap, model) for cap in (QS, QL) for model in (1, 2, 3, 4)}                   # 8
NAMED |= {("os_rowserial", cap, m) for cap in (QS, QL) for m in (1, 4, 16)}                              # 6
NAMED |= {("var_serial", cap, model) for cap in (QS, QL) for model in (1, 2, 3, 4)}                      # 2 x 4 (the model is an argument)
NAMED |= {("fused", r) for r in range(GATE_MAX_R + 1)} | {("two_pass",)}                                 # 5 + 1
assert len(NAMED) == 42 + 2 + 6 + 3 + 8 + 6 + 8 + 6

SCHEDULES = ("one_wg", "spread", "persistent")
FAMILIES = ("python", "numba", "variable")     # whose wavefront kernels take every schedule

# rowserial<kQueueLarge, 1> of both families is dead by arithmetic; nothing else is out of reach (see the degenerate palette below)
UNREACHED = {
    ("ed_rowserial", QL, 1): "M = 1 is chosen for K <= 64, kQueueLarge for n_inner > 64; a tree over K points has at most K - 1 <= 63 inner nodes",
    ("os_rowserial", QL, 1): "M = 1 is chosen for K <= 64, kQueueLarge for n_inner > 64; a tree over K points has at most K - 1 <= 63 inner nodes",
}

# ---- the trace line
_LINE = re.compile(r"dp_diffusion: kernel=(\w+) (.*?) ?schedule=(\w+) G=(\d+) grid=(\d+) waves=(\d+) lds=(\d+) K=(\d+) n_inner=(\d+) "
                   r"model=(\d+) numba=(\d) serpentine=(\d) repair=(\d)")
_GATE = re.compile(r"dp_variance_gate: kernel=(\w+) radius=(\d+) chunk=(\d+)")
Traced = collections.namedtuple("Traced", "instance schedule G grid waves lds K n_inner model numba serpentine repair")
TracedGate = collections.namedtuple("TracedGate", "instance radius chunk")


def _value(v):
    return _NAMES[v] if v in _NAMES else int(v)


def parse_trace(err):
    """the launches a stderr text names, in order: Traced for the diffusers, TracedGate for the gate"""
    out = []
    for line in err.splitlines():
        m = _LINE.search(line)
        if m:
            kernel, targs = m.group(1), {k: _value(v) for k, v in (kv.split("=") for kv in m.group(2).split())}
            nums = [int(v) for v in m.groups()[3:]]
            model = nums[6]
            if kernel == "ed_wavefront":
                inst = (kernel, targs["CAP"], targs["NT"], targs["EXACT"], targs["MAXW"], targs["NB"], targs["PALS"])
            elif kernel in ("ed_rowserial", "os_rowserial"):
                inst = (kernel, targs["CAP"], targs["M"])
            elif kernel == "ed_serial":
                inst = (kernel, targs["CAP"], targs["NB"])
            elif kernel == "var_wavefront":
                inst = (kernel, targs["CAP"], targs["MODEL"])
            elif kernel == "var_serial":
                inst = (kernel, targs["CAP"], model)
            else:
                raise ValueError(line)
            out.append(Traced(inst, m.group(3), *nums))
            continue
        m = _GATE.search(line)
        if m:
            kernel, radius, chunk = m.group(1), int(m.group(2)), int(m.group(3))
            out.append(TracedGate(("fused", min(radius, GATE_MAX_R)) if kernel == "fused" else (kernel,), radius, chunk))
    return out


# ---- the launchers' LDS conditions, restated
def _lists_in_lds(K):
    return K * 16 if K > 64 else 0      # (pal.K > 64 ? pal.K * 16 : 0): a lane holds several entries, their colours sit in LDS


def ed_rowserial_fits(w, K):
    """launch_error_diffusion: ((size_t)9 * w + 4) * sizeof(float) + (K > 64 ? K * 16 : 0) + 512 <= 158 * 1024"""
    return (9 * w + 4) * 4 + _lists_in_lds(K) + 512 <= LDS_LIMIT


def ed_rowserial_lds(w, K):
    """... and the dynamic LDS it then asks for: ((9 w + 3) & ~3) * sizeof(float) + (K > 64 ? K * 16 : 0)"""
    return ((9 * w + 3) & ~3) * 4 + _lists_in_lds(K)


def os_rowserial_fits(w, K):
    """launch_variable_diffusion: ((size_t)8 * w + 768) * sizeof(float) + (K > 64 ? K * 16 : 0) + 512 <= 158 * 1024"""
    return (8 * w + 768) * 4 + _lists_in_lds(K) + 512 <= LDS_LIMIT


def os_rowserial_lds(w, K):
    return (8 * w + 768) * 4 + _lists_in_lds(K)


def widest(fits, K):
    """the widest row for which `fits` holds (it is monotonic in w), by bisection on the launcher's own condition"""
    lo, hi = 1, WIDE_ROW
    assert fits(lo, K) and not fits(hi, K)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if fits(mid, K) else (lo, mid)
    return lo


# ---- palettes: spec -> (name, K).  n_inner of each is asserted in the CPU tier from dp_kdtree_build_host.
# ("palr", K): orc.palr(K), random colours: a balanced tree, 1 / 3 / 31 / 32 / 128 inner nodes at 16 / 40 / 256 / 300 / 1024 colours
# ("degenerate200",): tests/golden/degenerate200.npy, 200 float32 colours (135 distinct) whose tree has 76 inner nodes.  The tree
#   splits at the median VALUE, points below it to the left: a colour alone below a run of colours that coincide in the split
#   dimension up to the median position is split off by itself, and the run is split off next.  Nested over the three dimensions
#   (each run spreads in the remaining ones) that gives two inner nodes per colour split off, where a balanced tree spends ten
#   colours a leaf.  So 65 .. 256 colours CAN have more than 64 inner nodes, and rowserial<kQueueLarge, 4> is a case, not unreachable.
PALETTES = {"palr16": 16, "palr40": 40, "palr256": 256, "palr300": 300, "palr1024": 1024, "degenerate200": 200}
N_INNER = {"palr16": 1, "palr40": 3, "palr256": 31, "palr300": 32, "palr1024": 128, "degenerate200": 76}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def palette_f32(orc, name):
    """float32 [K, 3] as the tree sees it"""
    if name == "degenerate200":
        return np.ascontiguousarray(np.load(os.path.join(GOLDEN, "degenerate200.npy")), dtype=np.float32)
    return orc.prepare_palette(orc.palr(PALETTES[name]), False)[0]


def large_queue(name, any_k=True):
    """the launchers' kQueueLarge condition: n_inner > kQueueSmall, and for the wavefront / ed_serial kernels also K > 256"""
    return N_INNER[name] > QS or (any_k and PALETTES[name] > 256)


def search_kind(name):
    return "wide" if large_queue(name) else ("coarse" if PALETTES[name] <= 16 else "lists")


def rowserial_m(name):
    K = PALETTES[name]
    return 1 if K <= 64 else (4 if K <= 256 else 16)


# ---- tap sets: the reference's eight, and three custom ones dp_error_diffusion_u8 must re-sort into the reference's visiting order
# (taps, divisor) as orc.ed_kernel gives them; the named ones are looked up there by the GPU module
NAMED_TAPS = {"floyd_steinberg": 4, "atkinson": 6, "jjn": 12, "stucki": 12, "burkes": 7, "sierra": 10, "sierra_two_row": 7,
              "sierra_lite": 3}
CUSTOM_TAPS = {
    # five taps, unsorted, (2, 0) twice with two weights: the generic instance
    "custom5": ([(0, 2, 1), (-1, 1, 3), (2, 0, 5), (1, 0, 4), (2, 0, 2)], 16),
    # sixteen taps: the twelve causal positions of the window in a scrambled order, four of them twice with other weights
    "custom16": ([(1, 1, 5), (-2, 2, 1), (2, 0, 3), (0, 1, 7), (-1, 2, 2), (1, 0, 7), (2, 2, 1), (-2, 1, 3), (0, 2, 5), (2, 1, 3), (1, 2, 2),
                  (-1, 1, 5), (1, 0, 2), (0, 2, 1), (-2, 1, 2), (2, 2, 3)], 64),
    # taps on row dy = 2 only (row y + 1 receives nothing from row y)
    "row2": ([(-2, 2, 1), (2, 2, 1), (0, 2, 4), (-1, 2, 2), (1, 2, 2)], 10),
}
TAP_COUNTS = dict(NAMED_TAPS, **{k: len(v[0]) for k, v in CUSTOM_TAPS.items()})

# ---- CASES
Case = collections.namedtuple("Case", "id entry pal shape content params switches expect why")
# shape: (n, h, w); n may be ("cus", k): the device's CU count + k.  content: ("rnd", seed, distinct): `distinct` random frames dealt
# cyclically over the n frames (the oracle answers each once).  params: of the entry point.  expect: (instance, schedule).
CASES = []


def frames_of(shape, cus):
    n = shape[0]
    return (cus + n[1]) if isinstance(n, tuple) else n


def _add(id, entry, pal, shape, params, expect, why, content=None, switches=None):
    n = shape[0]
    distinct = 3 if isinstance(n, tuple) or n > 3 else n
    CASES.append(Case(id, entry, pal, shape, content or ("rnd", len(CASES) + 1, distinct), params, switches or {}, expect, why))


# -- ed_wavefront, python arithmetic: 3 search kinds x 11 tap sets x (four, sixteen) waves.  n_bands = ceil(h / 64): h = 130 gives 3 bands
# = 3 waves (nw <= 4: the four-wave instance), h = 321 gives 6 (the sixteen-wave instance); w = 23 < 64 rules the spread launch out,
# 1 or 2 frames <= CUs the persistent grid: one workgroup per frame
for _pal in ("palr16", "palr40", "palr300"):
    for _i, _taps in enumerate(list(NAMED_TAPS) + list(CUSTOM_TAPS)):
        for _h, _waves in ((130, 4), (321, MAX_WAVES)):
            _add(f"edw-{_pal}-{_taps}-h{_h}", "error_diffusion", _pal, (1 + _i % 2, _h, 23), dict(taps=_taps, serpentine=False),
                 (ed_wavefront(search_kind(_pal), TAP_COUNTS[_taps], _waves), "one_wg"),
                 f"{search_kind(_pal)} search, {TAP_COUNTS[_taps]} taps, {-(-_h // 64)} bands; w < 64: never spread")
# -- the numba arithmetic: one instance per workgroup size, nw <= 4 / nw = min(n_bands, 8)
for _h, _waves in ((130, 4), (321, NB_WAVES)):
    _add(f"edw-numba-h{_h}", "error_diffusion_numba", "palr40", (2, _h, 23), dict(taps="sierra", serpentine=False),
         (("ed_wavefront", QS, MAX_TAPS, False, _waves, True, 0), "one_wg"), f"{-(-_h // 64)} bands, numba arithmetic")
    _add(f"edw-hybrid-numba-h{_h}", "hybrid_numba", "palr16", (1, _h, 23), dict(lum_factor=1.0, col_factor=0.2),
         (("ed_wavefront", QS, MAX_TAPS, False, _waves, True, 0), "one_wg"), f"{-(-_h // 64)} bands, numba arithmetic with the hybrid transform")
# -- var_wavefront: 4 models x 2 queues (K = 300 > 256: kQueueLarge), h = 130: one workgroup of 3 waves
for _pal in ("palr40", "palr300"):
    for _model in (1, 2, 3, 4):
        _add(f"varw-{_pal}-model{_model}", "variable_diffusion", _pal, (2, 130, 23), dict(model=_model, serpentine=False),
             (("var_wavefront", QL if large_queue(_pal) else QS, _model), "one_wg"), "w < 60000 and not (model 4 and serpentine); w < 64: never spread")
# -- schedules, per family.  spread: n_frames * 2 <= CUs, n_bands >= 4, w >= 64: (1, 260, 67) has 5 bands, G = 4 workgroups of 2 waves
# (the four-wave instance) and the repair launch behind it.  persistent: G == 1, more than 4 waves, more frames than CUs:
# (CUs + 3, 321, 8) has 6 bands = 6 waves, w < 64
for _sched, _shape, _waves in (("spread", (1, 260, 67), 4), ("persistent", (("cus", 3), 321, 8), None)):
    _add(f"{_sched}-python", "error_diffusion", "palr40", _shape, dict(taps="floyd_steinberg", serpentine=False),
         (ed_wavefront("lists", 4, _waves or MAX_WAVES), _sched), "launch_error_diffusion, python arithmetic")
    _add(f"{_sched}-numba", "error_diffusion_numba", "palr16", _shape, dict(taps="floyd_steinberg", serpentine=False),
         (("ed_wavefront", QS, MAX_TAPS, False, _waves or NB_WAVES, True, 0), _sched), "launch_error_diffusion, numba arithmetic")
    _add(f"{_sched}-variable", "variable_diffusion", "palr40", _shape, dict(model=1, serpentine=False),
         (("var_wavefront", QS, 1), _sched), "launch_variable_diffusion")
# -- row-serial kernels at the edge of LDS: h = 4, two frames, the widest row that fits (the kernel at full LDS) and the next (the
# lane = frame kernel).  The widths come from the launchers' conditions (widest(...)), per palette size; M and the queue from the palette
ROWSERIAL_PALETTES = ("palr16", "palr256", "degenerate200", "palr300", "palr1024")
BOUNDARY = {}      # (family, palette) -> widest w that fits
for _pal in ROWSERIAL_PALETTES:
    _K = PALETTES[_pal]
    _big = N_INNER[_pal] > QS       # (the row-serial kernels and var_serial ask n_inner alone)
    BOUNDARY["ed", _pal] = _w = widest(ed_rowserial_fits, _K)
    _add(f"edr-{_pal}-w{_w}", "error_diffusion", _pal, (2, 4, _w), dict(taps="sierra", serpentine=True),
         (("ed_rowserial", QL if _big else QS, rowserial_m(_pal)), "rowserial"), f"(9 * {_w} + 4) * 4 + {_lists_in_lds(_K)} + 512 <= {LDS_LIMIT}")
    _add(f"edr-{_pal}-w{_w + 1}", "error_diffusion", _pal, (2, 4, _w + 1), dict(taps="sierra", serpentine=True),
         (("ed_serial", QL if large_queue(_pal) else QS, False), "serial"), f"(9 * {_w + 1} + 4) * 4 + {_lists_in_lds(_K)} + 512 > {LDS_LIMIT}")
    BOUNDARY["os", _pal] = _w = widest(os_rowserial_fits, _K)
    _add(f"osr-{_pal}-w{_w}", "variable_diffusion", _pal, (2, 4, _w), dict(model=4, serpentine=True),
         (("os_rowserial", QL if _big else QS, rowserial_m(_pal)), "rowserial"), f"(8 * {_w} + 768) * 4 + {_lists_in_lds(_K)} + 512 <= {LDS_LIMIT}")
    _add(f"osr-{_pal}-w{_w + 1}", "variable_diffusion", _pal, (2, 4, _w + 1), dict(model=4, serpentine=True),
         (("var_serial", QL if _big else QS, 4), "serial"), f"(8 * {_w + 1} + 768) * 4 + {_lists_in_lds(_K)} + 512 > {LDS_LIMIT}")
# -- the lane = frame kernels at w >= 60000: (2, 3, 60000), and (65, 2, 60000) = two blocks of 64 lanes, the second with one frame;
# w = 59999 with the same parameters stays on the wavefront kernel (h <= 3: one band, one wave) unless the scan is serpentine
SERIAL_SHAPES = ((2, 3, WIDE_ROW), (65, 2, WIDE_ROW))
for _pal in ("palr16", "palr300", "degenerate200"):
    _kind, _cap, _vcap = search_kind(_pal), QL if large_queue(_pal) else QS, QL if N_INNER[_pal] > QS else QS
    _variants = [("ed-raster", "error_diffusion", dict(taps="stucki", serpentine=False), ("ed_serial", _cap, False), ed_wavefront(_kind, 12, 4)),
                 ("ed-serp", "error_diffusion", dict(taps="stucki", serpentine=True), ("ed_serial", _cap, False), None),
                 ("numba", "error_diffusion_numba", dict(taps="burkes", serpentine=False), ("ed_serial", QS, True), ED_WAVEFRONT_NUMBA[0]),
                 ("hybrid-numba", "hybrid_numba", dict(lum_factor=1.0, col_factor=0.2), ("ed_serial", QS, True), ED_WAVEFRONT_NUMBA[0])]
    _variants += [(f"model{_m}", "variable_diffusion", dict(model=_m, serpentine=False), ("var_serial", _vcap, _m), ("var_wavefront", _cap, _m))
                  for _m in (1, 2, 3, 4)]
    _shapes = SERIAL_SHAPES
    if _pal == "degenerate200":
        # var_serial asks n_inner alone, so 300 random colours (32 inner nodes) leave it on kQueueSmall: the degenerate palette gives
        # var_serial<kQueueLarge> its four models.  The lane = frame kernel walks that tree with nothing to shorten the walk (some
        # 15 us a pixel): two rows of two frames
        _variants, _shapes = [v for v in _variants if v[1] == "variable_diffusion"], ((2, 2, WIDE_ROW),)
    for _name, _entry, _params, _serial, _wave in _variants:
        for _shape in _shapes:
            _add(f"serial-{_pal}-{_name}-n{_shape[0]}", _entry, _pal, _shape, _params, (_serial, "serial"), "w >= 60000")
        if _wave is not None:
            _add(f"serial-{_pal}-{_name}-w59999", _entry, _pal, _shapes[0][:2] + (WIDE_ROW - 1,), _params, (_wave, "one_wg"),
                 "w < 60000: one band, one wave")
# -- the gate: one fused instance per radius 0 .. 4 and the two-pass path from radius 5 (tests/test_gpu_variance_gate.py has the values)
for _r in range(GATE_MAX_R + 2):
    _add(f"gate-r{_r}", "variance_gate", "palr16", (2, 17, 65), dict(var_threshold=300.0, window_radius=_r),
         ((("fused", _r) if _r <= GATE_MAX_R else ("two_pass",)), None), "radius <= kGateMaxR: the fused kernel of that radius")
# -- the shared pieces of the band kernels (csrc/ed_band.hip.h) at the widths where they can go wrong; appended last, so that the rows
# above keep their content seeds.  PERIOD is 8 for the four-wave instance of error_diffusion, 16 for its sixteen-wave instance and for
# variable_diffusion; `why` names the helper path of each row.  (Three bands under one workgroup at w = 23 < 64 columns: the edw- and
# varw- rows above; more than 64 columns under one workgroup: the rows below.)
BAND_SHAPES = [((1, 3, _w), f"w = PERIOD {_w - _p:+d} = {_w}, one band: band_flush writes a row that ends {_p - _w:+d} columns from a period "
                            f"boundary byte by byte, and the pixel prefetch (band_fetch in var_wavefront) assembles the ends of the {9 * _w}-byte frame bytewise")
               for _p in (8, 16) for _w in (_p - 1, _p, _p + 1)]
BAND_TALL = [((1, 321, _w), f"w = 16 {_w - 16:+d}, six bands: BandWindow's 32 columns hang over both ends of the row in every period (band_col_margin on "
                            f"both sides); band_flush / band_advance at PERIOD = 16") for _w in (15, 16, 17)]
BAND_ODD = [((1, 1, 1), "no row above (band_tap_source: the zero slot for every tap) and a frame shorter than one dword: band_fetch and band_flush bytewise at both ends at once"),
            ((1, 65, 9), "the second band has a single row: BandWindow / band_poll with one lane at work, band_finished after w + 0 * skew steps"),
            ((2, 130, 70), "three bands under one workgroup, wider than the 64-column ring of the rows above: BandWindow columns wrap in s_vring; whole-dword band_flush")]
for _shape, _why in [s for s in BAND_SHAPES if s[0][2] in (7, 8, 9)] + BAND_TALL + BAND_ODD:
    _waves = 4 if _shape[1] <= 256 else MAX_WAVES
    _add(f"band-ed-{_shape[0]}x{_shape[1]}x{_shape[2]}", "error_diffusion", "palr40", _shape, dict(taps="floyd_steinberg", serpentine=False),
         (ed_wavefront("lists", 4, _waves), "one_wg"), _why)
for _shape, _why in [s for s in BAND_SHAPES if s[0][2] in (15, 16, 17)] + BAND_TALL + BAND_ODD:
    _add(f"band-var-{_shape[0]}x{_shape[1]}x{_shape[2]}", "variable_diffusion", "palr40", _shape, dict(model=1, serpentine=False),
         (("var_wavefront", QS, 1), "one_wg"), _why)
# model 3's gate bytes go through band_fetch as well (one byte per pixel): a map of tests/test_gpu_diffusion_instances.py: _gate_patterns
_add("band-var-gate-2x130x70", "variable_diffusion", "palr40", (2, 130, 70), dict(model=3, serpentine=False, gate_pattern="checkerboard"),
     (("var_wavefront", QS, 3), "one_wg"), "band_fetch<4> of the gate bytes, a period ahead, at both ends of the map and across three bands")

assert len({c.id for c in CASES}) == len(CASES)
