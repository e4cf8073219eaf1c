"""Everything the deep self-test shows of its three parts at once, without a GPU, against recorded
literals: `to_dict()`, `describe_failure()`, the notes, `failed_cus`, `fenceable`, the command's
text and --json output (with --fence too) and the /metrics lines, of a run in which the sweep, a
matrix path, the vector ALU, the scalar unit and HBM all fail, of a masked run that misses a CU, and
of a probe without the vector-ALU and scalar bindings; and both parsers' help and the errors of
their three flags. The literals in `EXPECTED` were recorded from the code as it stood before the
parts were put behind one table; `_observe()` is what recorded them."""
import json
import types

import pytest

from nanogpu.agent.metrics import render as render_metrics
from nanogpu.agent.node import build_parser
from nanogpu.probe import selftest as S
from nanogpu.probe.selftest_paths import PATHS
from nanogpu.probe.selftest_scalar import GROUPS as SCALAR_GROUPS
from nanogpu.probe.selftest_valu import GROUPS as VALU_GROUPS
from nanogpu.topology.model import synthetic_mi355x

GIB = 1 << 30
HASH = 0x1234ABCD


def _hw(key, simd=0):
    return (key << 8) | (simd << 4)


class _FakeProbe:
    """8 XCDs x 32 CU keys. Every launch leaves out the CUs in `hidden`; the lists below add failing
    records, each only when its CU is in the mask and its path or group was asked for."""
    sweep_bad = [(3, 17, 0b0001, -1), (5, 2, 0x10, 40959)]              # (xcc, key, fail bits, LDS dword)
    path_bad = [(1, 4, "fp8")]
    valu_bad = [(2, 9, "regs", 0x10 << (70 >> 6), 0, 5, 70, HASH),      # (.., kind, fail, group bits, slot, thread, hash)
                (2, 9, "cvt", 1, 1 << VALU_GROUPS.index("cvt"), -1, -1, HASH),
                (6, 30, "approx", 0, 0, -1, -1, HASH ^ 1)]
    scalar_bad = [(4, 1, "smem", 0x10 << 3, 4095, 3, 1), (4, 1, "sregs", 0x100, 0, 0, 0)]   # (.., kind, fail, index, wave, which)
    hbm_errors = 2

    def __init__(self, cus=256, hidden=(), failing=True):
        self.cus, self.hidden, self.failing = cus, set(hidden), failing
        self.calls = []

    def device_count(self):
        return 1

    def device_props(self, dev):
        return {"cus": self.cus}

    def mem_info(self, dev):
        return 3 * GIB, 288 * GIB

    def _keys(self, mask):
        keys = [(i % 8, i // 8) for i in range(self.cus) if not mask or (mask[i // 32] >> (i % 32)) & 1]
        return [k for k in keys if k not in self.hidden]

    def _sweep_records(self, mask):
        keys = self._keys(mask)
        recs = [(x, _hw(k), 0, 0xF, -1) for x, k in keys]
        if self.failing:
            recs += [(x, _hw(k), fail, 0xF, off) for x, k, fail, off in self.sweep_bad if (x, k) in keys]
        return recs

    def cu_sweep(self, dev, mask, rounds, seed, inject=None):
        self.calls.append(("sweep", rounds))
        return {"records": self._sweep_records(mask), "lds_bytes": 163840, "ms": 0.25}

    def cu_sweep_paths(self, dev, mask, rounds, seed, paths, inject=None):
        self.calls.append(("paths", rounds))
        keys = self._keys(mask)
        recs = [r + (0, 0) for r in self._sweep_records(mask)]
        if self.failing:
            recs += [(x, _hw(k), 0, 0xF, -1, 1 << PATHS.index(name), 0b0001)
                     for x, k, name in self.path_bad if name in paths and (x, k) in keys]
        return {"records": recs, "paths": list(PATHS), "checked": list(paths), "lds_bytes": 163840, "ms": 0.25}

    def cu_sweep_valu(self, dev, mask, rounds, seed, groups, inject=None, corrupt_expected=None):
        self.calls.append(("valu", rounds))
        keys = self._keys(mask)
        recs = [(x, _hw(k), 0, 0xF, 0, -1, -1, HASH) for x, k in keys]
        if self.failing:
            recs += [(x, _hw(k), fail, 0xF, gbits, slot, thread, ahash)
                     for x, k, kind, fail, gbits, slot, thread, ahash in self.valu_bad if kind in groups and (x, k) in keys]
        return {"records": recs, "groups": list(VALU_GROUPS), "checked": list(groups), "reg_slots": 448, "regs_per_lane": 512,
                "scratch_bytes": 0, "ms": 0.5}

    def cu_sweep_scalar(self, dev, mask, rounds, seed, groups, inject=None, corrupt_expected=None):
        self.calls.append(("scalar", rounds))
        keys = self._keys(mask)
        recs = [(x, _hw(k), 0, 0xF, 0, -1, -1, -1) for x, k in keys]
        if self.failing:
            recs += [(x, _hw(k), fail, 0xF, 0, index, wave, which)
                     for x, k, kind, fail, index, wave, which in self.scalar_bad if kind in groups and (x, k) in keys]
        return {"records": recs, "groups": list(SCALAR_GROUPS), "checked": list(groups), "sreg_slots": 88, "num_regs": 16,
                "scratch_bytes": 0, "ms": 0.3}

    def hbm_pattern_check(self, dev, nbytes, seed, passes=2, corrupt=(), verify_seed=None, cu_mask=None):
        e = self.hbm_errors if self.failing else 0
        return {"bytes": nbytes, "errors": e, "first": [(4096 * 16, 0x11, 0x10)] if e else [], "fill_gbs": 5000.0,
                "verify_gbs": 6000.0}


class _OldProbe(_FakeProbe):
    cu_sweep_valu = property()          # hasattr() is False
    cu_sweep_scalar = property()


def _shown(rep) -> dict:
    return {"to_dict": dict(rep.to_dict(), seconds=0), "describe_failure": rep.describe_failure(), "notes": list(rep.notes),
            "failed_cus": sorted(S.failed_cus(rep)), "fenceable": S.fenceable(rep)}


def _main_output(mp, capsys, P, argv) -> str:
    import nanogpu.native

    mp.setattr(nanogpu.native, "probe", lambda required=False, build=False: P)
    capsys.readouterr()
    assert S.main(argv) == 1
    return capsys.readouterr().out


def _exits(capsys, call, code: int) -> str:
    """What a command that ends in SystemExit(code) printed, its white space as single blanks: the help (code 0), or
    the error without the usage lines before it (code 2)."""
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        call()
    assert e.value.code == code
    got = capsys.readouterr()
    return " ".join(got.out.split()) if code == 0 else " ".join(got.err.split()).split(" error: ", 1)[1]


def _observe(capsys) -> dict:
    """What `EXPECTED` holds, from the code as it is now."""
    out = {}
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(S, "time", types.SimpleNamespace(perf_counter=lambda: 0.0, time=lambda: 0.001))   # seconds 0, seed 1
        P = _FakeProbe()
        rep = S.deep_selftest(P, 0, hbm_bytes=GIB, seed=1, paths="all", valu="all", scalar="all")
        out["all_fail"] = dict(_shown(rep), calls=list(P.calls))
        P = _FakeProbe(hidden=[(3, 5)], failing=False)
        rep = S.deep_selftest(P, 0, cu_mask_bits=list(range(40, 48)), hbm_bytes=1 << 26, seed=1, paths="all", valu="all",
                              scalar="all")
        out["masked"] = dict(_shown(rep), calls=list(P.calls))
        P = _OldProbe()
        rep = S.deep_selftest(P, 0, hbm_bytes=GIB, seed=1, paths="all", valu="all", scalar="all")
        out["old_probe"] = dict(_shown(rep), calls=list(P.calls))
        argv = ["--hbm-mib", "1024", "--paths", "all", "--valu", "all", "--scalar", "all"]
        out["main_text"] = _main_output(mp, capsys, _FakeProbe(), argv)
        out["main_json"] = json.loads(_main_output(mp, capsys, _FakeProbe(), argv + ["--json"]))
        out["main_fence_text"] = _main_output(mp, capsys, _FakeProbe(), argv + ["--fence", "2"])
        with_fence = json.loads(_main_output(mp, capsys, _FakeProbe(), argv + ["--fence", "2", "--json"]))
        assert list(with_fence)[-1] == "fence"
        out["main_fence_json_fence"] = with_fence.pop("fence")
        assert repr(with_fence) == repr(out["main_json"])
        # without the HBM errors the failure is a CU's to fence: six units fail again when swept alone
        quiet = _FakeProbe()
        quiet.hbm_errors = 0
        out["main_fence_units_text"] = _main_output(mp, capsys, quiet, argv + ["--fence", "6"])
        mp.setenv("COLUMNS", "100")
        out["main_help"] = _exits(capsys, lambda: S.main(["--help"]), 0)
        out["agent_help"] = " ".join(build_parser().format_help().split())
        for flag, bad in (("paths", "fp8,nope"), ("valu", "fma32,nope"), ("scalar", "add,nope")):
            out[f"main_{flag}_error"] = _exits(capsys, lambda: S.main([f"--{flag}", bad]), 2)
            out[f"agent_{flag}_error"] = _exits(capsys, lambda: build_parser().parse_args([f"--selftest-{flag}", bad]), 2)
            out[f"agent_{flag}_empty"] = _exits(capsys, lambda: build_parser().parse_args([f"--selftest-{flag}", ""]), 2)
        a = build_parser().parse_args([])
        out["agent_defaults"] = [a.selftest_paths, a.selftest_valu, a.selftest_scalar]
    stats = {"reports": {0: out["all_fail"]["to_dict"]}, "at": {0: 0.0}, "runs": {(0, "fail"): 1}}
    text = render_metrics(synthetic_mi355x(1), None, None, "/nonexistent", stats)
    out["metrics"] = [line for line in text.splitlines() if "nanogpu_selftest_" in line]
    return out


def test_every_output_of_the_three_parts_is_as_recorded(capsys):
    seen = _observe(capsys)
    assert list(seen) == list(EXPECTED)
    for name in EXPECTED:
        assert seen[name] == EXPECTED[name], name
        assert repr(seen[name]) == repr(EXPECTED[name]), name       # the order of keys is part of what --json shows


EXPECTED = {'all_fail': {'to_dict': {'device': 0,
                          'ok': False,
                          'seconds': 0,
                          'sweep': {'cus_seen': 256,
                                    'cus_expected': 256,
                                    'per_xcd': {0: 32, 1: 32, 2: 32, 3: 32, 4: 32, 5: 32, 6: 32, 7: 32},
                                    'failed': [{'xcc': 3, 'cu_key': 17, 'kinds': ['mfma'], 'lds_bad_off': -1},
                                               {'xcc': 5, 'cu_key': 2, 'kinds': ['lds'], 'lds_bad_off': 40959}],
                                    'uncovered': [],
                                    'cus_uncovered': 0,
                                    'simds_seen_min': 4,
                                    'lds_bytes': 163840,
                                    'launches': 1,
                                    'ms': 0.25},
                          'hbm': {'bytes': 1073741824,
                                  'errors': 2,
                                  'first': [(65536, 17, 16)],
                                  'fill_gbs': 5000.0,
                                  'verify_gbs': 6000.0},
                          'error': None,
                          'masked': False,
                          'seed': 1,
                          'notes': [],
                          'paths': {'checked': ['f16', 'fp8', 'bf8', 'i8', 'mxfp8', 'mxfp6', 'mxfp4', 'f32', 'f64'],
                                    'failed': {'fp8': [[1, 4]]}},
                          'valu': {'checked': ['fma32', 'fma64', 'pkfma16', 'pkfma32', 'addmul32', 'int32', 'int64',
                                               'bits', 'dot', 'cvt', 'xlane', 'approx', 'regs'],
                                   'failed': {'cvt': [[2, 9]], 'regs': [[2, 9]], 'approx': [[6, 30]]},
                                   'cus': [{'xcc': 2,
                                            'cu_key': 9,
                                            'kinds': ['cvt', 'regs'],
                                            'waves': 3,
                                            'bad_slot': 5,
                                            'bad_wave': 1,
                                            'bad_lane': 6},
                                           {'xcc': 6,
                                            'cu_key': 30,
                                            'kinds': ['approx'],
                                            'waves': 15,
                                            'bad_slot': -1,
                                            'bad_wave': -1,
                                            'bad_lane': -1}],
                                   'reg_slots': 448,
                                   'ms': 0.5},
                          'scalar': {'checked': ['add', 'mul', 'shift', 'logic', 'bits', 'cmp', 'vcc', 'smem',
                                                 'sregs'],
                                     'failed': {'smem': [[4, 1]], 'sregs': [[4, 1]]},
                                     'cus': [{'xcc': 4,
                                              'cu_key': 1,
                                              'kinds': ['smem', 'sregs'],
                                              'waves': 9,
                                              'bad_slot': 0,
                                              'bad_slot_wave': 0,
                                              'bad_word': 4095,
                                              'bad_word_wave': 3}],
                                     'sreg_slots': 88,
                                     'ms': 0.3}},
              'describe_failure': 'CU (xcc 3, key 0x11) mfma; CU (xcc 5, key 0x2) lds at LDS dword 40959; matrix '
                                  'path fp8 on CU (xcc 1, key 0x4); vector ALU cvt+regs on CU (xcc 2, key 0x9) at '
                                  'slot 5, wave 1 lane 6; vector ALU approx on CU (xcc 6, key 0x1e); scalar unit '
                                  'smem+sregs on CU (xcc 4, key 0x1), at slot 0, wave 0, at word 4095, wave 3; 2 HBM '
                                  'elements wrong, first at byte 65536 (expected 0x00000011, got 0x00000010)',
              'notes': [],
              'failed_cus': [(1, 4), (2, 9), (3, 17), (4, 1), (5, 2), (6, 30)],
              'fenceable': False,
              'calls': [('paths', 4), ('valu', 4), ('scalar', 4)]},
 'masked': {'to_dict': {'device': 0,
                        'ok': True,
                        'seconds': 0,
                        'sweep': {'cus_seen': 7,
                                  'cus_expected': 8,
                                  'per_xcd': {0: 1, 1: 1, 2: 1, 4: 1, 5: 1, 6: 1, 7: 1},
                                  'failed': [],
                                  'uncovered': [],
                                  'cus_uncovered': 1,
                                  'simds_seen_min': 4,
                                  'lds_bytes': 163840,
                                  'launches': 3,
                                  'ms': 0.25},
                        'hbm': {'bytes': 67108864,
                                'errors': 0,
                                'first': [],
                                'fill_gbs': 5000.0,
                                'verify_gbs': 6000.0},
                        'error': None,
                        'masked': True,
                        'seed': 1,
                        'notes': ['1 CUs not reached by the vector-ALU launches',
                                  '1 CUs not reached by the scalar launches', '1 CUs not reached in 3 launches'],
                        'paths': {'checked': ['f16', 'fp8', 'bf8', 'i8', 'mxfp8', 'mxfp6', 'mxfp4', 'f32', 'f64'],
                                  'failed': {}},
                        'valu': {'checked': ['fma32', 'fma64', 'pkfma16', 'pkfma32', 'addmul32', 'int32', 'int64',
                                             'bits', 'dot', 'cvt', 'xlane', 'approx', 'regs'],
                                 'failed': {},
                                 'cus': [],
                                 'reg_slots': 448,
                                 'ms': 0.5},
                        'scalar': {'checked': ['add', 'mul', 'shift', 'logic', 'bits', 'cmp', 'vcc', 'smem', 'sregs'],
                                   'failed': {},
                                   'cus': [],
                                   'sreg_slots': 88,
                                   'ms': 0.3}},
            'describe_failure': '',
            'notes': ['1 CUs not reached by the vector-ALU launches', '1 CUs not reached by the scalar launches',
                      '1 CUs not reached in 3 launches'],
            'failed_cus': [],
            'fenceable': False,
            'calls': [('paths', 4), ('valu', 4), ('scalar', 4), ('paths', 8), ('valu', 8), ('scalar', 8),
                      ('paths', 16), ('valu', 16), ('scalar', 16)]},
 'old_probe': {'to_dict': {'device': 0,
                           'ok': False,
                           'seconds': 0,
                           'sweep': {'cus_seen': 256,
                                     'cus_expected': 256,
                                     'per_xcd': {0: 32, 1: 32, 2: 32, 3: 32, 4: 32, 5: 32, 6: 32, 7: 32},
                                     'failed': [{'xcc': 3, 'cu_key': 17, 'kinds': ['mfma'], 'lds_bad_off': -1},
                                                {'xcc': 5, 'cu_key': 2, 'kinds': ['lds'], 'lds_bad_off': 40959}],
                                     'uncovered': [],
                                     'cus_uncovered': 0,
                                     'simds_seen_min': 4,
                                     'lds_bytes': 163840,
                                     'launches': 1,
                                     'ms': 0.25},
                           'hbm': {'bytes': 1073741824,
                                   'errors': 2,
                                   'first': [(65536, 17, 16)],
                                   'fill_gbs': 5000.0,
                                   'verify_gbs': 6000.0},
                           'error': None,
                           'masked': False,
                           'seed': 1,
                           'notes': ['this probe has no cu_sweep_valu: no vector-ALU group was checked',
                                     'this probe has no cu_sweep_scalar: no scalar group was checked'],
                           'paths': {'checked': ['f16', 'fp8', 'bf8', 'i8', 'mxfp8', 'mxfp6', 'mxfp4', 'f32', 'f64'],
                                     'failed': {'fp8': [[1, 4]]}}},
               'describe_failure': 'CU (xcc 3, key 0x11) mfma; CU (xcc 5, key 0x2) lds at LDS dword 40959; matrix '
                                   'path fp8 on CU (xcc 1, key 0x4); 2 HBM elements wrong, first at byte 65536 '
                                   '(expected 0x00000011, got 0x00000010)',
               'notes': ['this probe has no cu_sweep_valu: no vector-ALU group was checked',
                         'this probe has no cu_sweep_scalar: no scalar group was checked'],
               'failed_cus': [(1, 4), (3, 17), (5, 2)],
               'fenceable': False,
               'calls': [('paths', 4)]},
 'main_text': 'device 0: FAILED in 0.000 s\n'
              '  CUs checked 256/256 (per XCD {0: 32, 1: 32, 2: 32, 3: 32, 4: 32, 5: 32, 6: 32, 7: 32}), 2 failed, 0 '
              'not reached, LDS 163840 B per CU, sweep 0.250 ms in 1 launch(es)\n'
              '  matrix paths f16, fp8, bf8, i8, mxfp8, mxfp6, mxfp4, f32, f64: fp8 failed on 1 CU(s)\n'
              '  vector ALU fma32, fma64, pkfma16, pkfma32, addmul32, int32, int64, bits, dot, cvt, xlane, approx, '
              'regs (448 registers a lane, 0.500 ms): approx failed on 1 CU(s), cvt failed on 1 CU(s), regs failed '
              'on 1 CU(s)\n'
              '  scalar unit add, mul, shift, logic, bits, cmp, vcc, smem, sregs (88 registers a wave, 0.300 ms): '
              'smem failed on 1 CU(s), sregs failed on 1 CU(s)\n'
              '  HBM 1073741824 B x 2 passes: 2 errors, fill 5000 GB/s, verify 6000 GB/s, 1 launch(es) a pass\n'
              '  CU (xcc 3, key 0x11) mfma; CU (xcc 5, key 0x2) lds at LDS dword 40959; matrix path fp8 on CU (xcc '
              '1, key 0x4); vector ALU cvt+regs on CU (xcc 2, key 0x9) at slot 5, wave 1 lane 6; vector ALU approx '
              'on CU (xcc 6, key 0x1e); scalar unit smem+sregs on CU (xcc 4, key 0x1), at slot 0, wave 0, at word '
              '4095, wave 3; 2 HBM elements wrong, first at byte 65536 (expected 0x00000011, got 0x00000010)\n',
 'main_json': {'device': 0,
               'ok': False,
               'seconds': 0.0,
               'sweep': {'cus_seen': 256,
                         'cus_expected': 256,
                         'per_xcd': {'0': 32, '1': 32, '2': 32, '3': 32, '4': 32, '5': 32, '6': 32, '7': 32},
                         'failed': [{'xcc': 3, 'cu_key': 17, 'kinds': ['mfma'], 'lds_bad_off': -1},
                                    {'xcc': 5, 'cu_key': 2, 'kinds': ['lds'], 'lds_bad_off': 40959}],
                         'uncovered': [],
                         'cus_uncovered': 0,
                         'simds_seen_min': 4,
                         'lds_bytes': 163840,
                         'launches': 1,
                         'ms': 0.25},
               'hbm': {'bytes': 1073741824,
                       'errors': 2,
                       'first': [[65536, 17, 16]],
                       'fill_gbs': 5000.0,
                       'verify_gbs': 6000.0},
               'error': None,
               'masked': False,
               'seed': 1,
               'notes': [],
               'paths': {'checked': ['f16', 'fp8', 'bf8', 'i8', 'mxfp8', 'mxfp6', 'mxfp4', 'f32', 'f64'],
                         'failed': {'fp8': [[1, 4]]}},
               'valu': {'checked': ['fma32', 'fma64', 'pkfma16', 'pkfma32', 'addmul32', 'int32', 'int64', 'bits',
                                    'dot', 'cvt', 'xlane', 'approx', 'regs'],
                        'failed': {'cvt': [[2, 9]], 'regs': [[2, 9]], 'approx': [[6, 30]]},
                        'cus': [{'xcc': 2,
                                 'cu_key': 9,
                                 'kinds': ['cvt', 'regs'],
                                 'waves': 3,
                                 'bad_slot': 5,
                                 'bad_wave': 1,
                                 'bad_lane': 6},
                                {'xcc': 6,
                                 'cu_key': 30,
                                 'kinds': ['approx'],
                                 'waves': 15,
                                 'bad_slot': -1,
                                 'bad_wave': -1,
                                 'bad_lane': -1}],
                        'reg_slots': 448,
                        'ms': 0.5},
               'scalar': {'checked': ['add', 'mul', 'shift', 'logic', 'bits', 'cmp', 'vcc', 'smem', 'sregs'],
                          'failed': {'smem': [[4, 1]], 'sregs': [[4, 1]]},
                          'cus': [{'xcc': 4,
                                   'cu_key': 1,
                                   'kinds': ['smem', 'sregs'],
                                   'waves': 9,
                                   'bad_slot': 0,
                                   'bad_slot_wave': 0,
                                   'bad_word': 4095,
                                   'bad_word_wave': 3}],
                          'sreg_slots': 88,
                          'ms': 0.3}},
 'main_fence_text': 'device 0: FAILED in 0.000 s\n'
                    '  CUs checked 256/256 (per XCD {0: 32, 1: 32, 2: 32, 3: 32, 4: 32, 5: 32, 6: 32, 7: 32}), 2 '
                    'failed, 0 not reached, LDS 163840 B per CU, sweep 0.250 ms in 1 launch(es)\n'
                    '  matrix paths f16, fp8, bf8, i8, mxfp8, mxfp6, mxfp4, f32, f64: fp8 failed on 1 CU(s)\n'
                    '  vector ALU fma32, fma64, pkfma16, pkfma32, addmul32, int32, int64, bits, dot, cvt, xlane, '
                    'approx, regs (448 registers a lane, 0.500 ms): approx failed on 1 CU(s), cvt failed on 1 CU(s), '
                    'regs failed on 1 CU(s)\n'
                    '  scalar unit add, mul, shift, logic, bits, cmp, vcc, smem, sregs (88 registers a wave, 0.300 '
                    'ms): smem failed on 1 CU(s), sregs failed on 1 CU(s)\n'
                    '  HBM 1073741824 B x 2 passes: 2 errors, fill 5000 GB/s, verify 6000 GB/s, 1 launch(es) a pass\n'
                    '  CU (xcc 3, key 0x11) mfma; CU (xcc 5, key 0x2) lds at LDS dword 40959; matrix path fp8 on CU '
                    '(xcc 1, key 0x4); vector ALU cvt+regs on CU (xcc 2, key 0x9) at slot 5, wave 1 lane 6; vector '
                    'ALU approx on CU (xcc 6, key 0x1e); scalar unit smem+sregs on CU (xcc 4, key 0x1), at slot 0, '
                    'wave 0, at word 4095, wave 3; 2 HBM elements wrong, first at byte 65536 (expected 0x00000011, '
                    'got 0x00000010)\n'
                    "  would fence nothing: a HIP error, HBM errors or a garbled record are not a CU's to fence\n",
 'main_fence_json_fence': {'units': [],
                           'cus': {},
                           'reason': "a HIP error, HBM errors or a garbled record are not a CU's to fence",
                           'seconds': 0.0},
 'main_fence_units_text': 'device 0: FAILED in 0.000 s\n'
                          '  CUs checked 256/256 (per XCD {0: 32, 1: 32, 2: 32, 3: 32, 4: 32, 5: 32, 6: 32, 7: 32}), '
                          '2 failed, 0 not reached, LDS 163840 B per CU, sweep 0.250 ms in 1 launch(es)\n'
                          '  matrix paths f16, fp8, bf8, i8, mxfp8, mxfp6, mxfp4, f32, f64: fp8 failed on 1 CU(s)\n'
                          '  vector ALU fma32, fma64, pkfma16, pkfma32, addmul32, int32, int64, bits, dot, cvt, '
                          'xlane, approx, regs (448 registers a lane, 0.500 ms): approx failed on 1 CU(s), cvt '
                          'failed on 1 CU(s), regs failed on 1 CU(s)\n'
                          '  scalar unit add, mul, shift, logic, bits, cmp, vcc, smem, sregs (88 registers a wave, '
                          '0.300 ms): smem failed on 1 CU(s), sregs failed on 1 CU(s)\n'
                          '  HBM 1073741824 B x 2 passes: 0 errors, fill 5000 GB/s, verify 6000 GB/s, 1 launch(es) a '
                          'pass\n'
                          '  CU (xcc 3, key 0x11) mfma; CU (xcc 5, key 0x2) lds at LDS dword 40959; matrix path fp8 '
                          'on CU (xcc 1, key 0x4); vector ALU cvt+regs on CU (xcc 2, key 0x9) at slot 5, wave 1 lane '
                          '6; vector ALU approx on CU (xcc 6, key 0x1e); scalar unit smem+sregs on CU (xcc 4, key '
                          '0x1), at slot 0, wave 0, at word 4095, wave 3\n'
                          '  would fence 6 unit(s) in 0.000 s:\n'
                          '    unit 1: (xcc 0, key 0x1), (xcc 1, key 0x1), (xcc 2, key 0x1), (xcc 3, key 0x1), (xcc '
                          '4, key 0x1), (xcc 5, key 0x1), (xcc 6, key 0x1), (xcc 7, key 0x1)\n'
                          '    unit 2: (xcc 0, key 0x2), (xcc 1, key 0x2), (xcc 2, key 0x2), (xcc 3, key 0x2), (xcc '
                          '4, key 0x2), (xcc 5, key 0x2), (xcc 6, key 0x2), (xcc 7, key 0x2)\n'
                          '    unit 4: (xcc 0, key 0x4), (xcc 1, key 0x4), (xcc 2, key 0x4), (xcc 3, key 0x4), (xcc '
                          '4, key 0x4), (xcc 5, key 0x4), (xcc 6, key 0x4), (xcc 7, key 0x4)\n'
                          '    unit 9: (xcc 0, key 0x9), (xcc 1, key 0x9), (xcc 2, key 0x9), (xcc 3, key 0x9), (xcc '
                          '4, key 0x9), (xcc 5, key 0x9), (xcc 6, key 0x9), (xcc 7, key 0x9)\n'
                          '    unit 17: (xcc 0, key 0x11), (xcc 1, key 0x11), (xcc 2, key 0x11), (xcc 3, key 0x11), '
                          '(xcc 4, key 0x11), (xcc 5, key 0x11), (xcc 6, key 0x11), (xcc 7, key 0x11)\n'
                          '    unit 30: (xcc 0, key 0x1e), (xcc 1, key 0x1e), (xcc 2, key 0x1e), (xcc 3, key 0x1e), '
                          '(xcc 4, key 0x1e), (xcc 5, key 0x1e), (xcc 6, key 0x1e), (xcc 7, key 0x1e)\n',
 'main_help': 'usage: python -m nanogpu.probe.selftest [-h] [--device DEVICE] [--hbm-mib HBM_MIB] [--paths all|LIST] '
              "[--valu all|LIST] [--scalar all|LIST] [--fence N] [--json] deep self-test of one GPU: every CU's MFMA "
              'and LDS, and HBM options: -h, --help show this help message and exit --device DEVICE --hbm-mib '
              'HBM_MIB HBM to pattern-check in MiB (default 1024; 0: all free memory less 2 GiB) --paths all|LIST '
              "matrix paths every CU also runs: 'all' or a comma-separated list of f16, fp8, bf8, i8, mxfp8, mxfp6, "
              "mxfp4, f32, f64 --valu all|LIST vector-ALU groups, 'approx' and 'regs' every CU also runs: 'all' or a "
              "comma- separated list --scalar all|LIST scalar-ALU groups, 'vcc', 'smem' and 'sregs' every CU also "
              "runs: 'all' or a comma-separated list --fence N after a failed sweep, print the CU-mask units (at "
              'most N) and CUs an agent started with --selftest-fence N would fence; changes nothing on the device '
              'or the node --json',
 'agent_help': 'usage: nanogpu-agent [-h] [--node-name NODE_NAME] [--sysfs-root SYSFS_ROOT] [--no-amdsmi] '
               '[--calibrate] [--advertise {device-plugin,status}] [--plugin-dir PLUGIN_DIR] [--kube-api KUBE_API] '
               '[--kubeconfig KUBECONFIG] [--print] [--selftest] [--selftest-deep] [--selftest-paths all|LIST] '
               '[--selftest-valu all|LIST] [--selftest-scalar all|LIST] [--selftest-fence UNITS] '
               '[--selftest-fence-reset] [--selftest-hbm-mib SELFTEST_HBM_MIB] [--selftest-period SELFTEST_PERIOD] '
               '[--metrics-port METRICS_PORT] [--pod-resources-socket POD_RESOURCES_SOCKET] [--reconcile-period '
               'RECONCILE_PERIOD] MI355X node agent for nano-gpu-scheduler options: -h, --help show this help '
               'message and exit --node-name NODE_NAME --sysfs-root SYSFS_ROOT --no-amdsmi --calibrate run the HIP '
               'probe (HBM GB/s) before publishing --advertise {device-plugin,status} --plugin-dir PLUGIN_DIR '
               '--kube-api KUBE_API --kubeconfig KUBECONFIG --print print the topology annotation and exit '
               '--selftest run the HIP self-test (HBM copy + MFMA tile) on every device at start-up --selftest-deep '
               'the start-up self-test checks every CU (MFMA pipes, LDS) and the free HBM with an address-derived '
               'pattern instead of one tile and 16 MiB (implies --selftest) --selftest-paths all|LIST the deep '
               "self-test also runs an exact MFMA chain of these matrix paths on every CU: 'all' or a "
               'comma-separated list of f16, fp8, bf8, i8, mxfp8, mxfp6, mxfp4, f32, f64 (implies --selftest-deep; '
               'start-up and periodic runs alike) --selftest-valu all|LIST the deep self-test also runs, on all four '
               'SIMDs of every CU, exact chains of vector-ALU instructions, the transcendentals and a pattern test '
               "of the vector register file: 'all' or a comma-separated list of fma32, fma64, pkfma16, pkfma32, "
               'addmul32, int32, int64, bits, dot, cvt, xlane, approx, regs (implies --selftest-deep; start-up and '
               'periodic runs alike) --selftest-scalar all|LIST the deep self-test also runs, on all four waves of '
               'every CU, exact chains of scalar-ALU instructions, the vector / scalar boundary, scalar loads of '
               "every width and a pattern test of the wave's scalar registers: 'all' or a comma-separated list of "
               'add, mul, shift, logic, bits, cmp, vcc, smem, sregs (implies --selftest-deep; start-up and periodic '
               'runs alike) --selftest-fence UNITS a whole GPU (SPX) whose deep self-test fails on CUs that fail '
               'again when swept alone stays Healthy and loses the CU-mask units (8 CUs, one per XCD, each) that '
               'hold them: at most UNITS a device, those carried over a restart included (0: off; implies '
               "--selftest-deep; needs the device plugin) --selftest-fence-reset start without the fences the node's "
               "topology annotation holds --selftest-hbm-mib SELFTEST_HBM_MIB cap of the deep self-test's HBM check "
               'in MiB (0: all free HBM less 2 GiB); only devices without a grant are checked --selftest-period '
               'SELFTEST_PERIOD seconds between deep re-tests of the CUs no tenant holds (0: off) --metrics-port '
               'METRICS_PORT device / pod / container GPU metrics on :PORT/metrics (0: off) --pod-resources-socket '
               "POD_RESOURCES_SOCKET kubelet's pod-resources API: the grants are checked against it ('' : off) "
               '--reconcile-period RECONCILE_PERIOD seconds between pod-resources checks (0: off)',
 'main_paths_error': "unknown matrix path(s) ['nope']: choose from f16, fp8, bf8, i8, mxfp8, mxfp6, mxfp4, f32, f64 "
                     "or 'all'",
 'agent_paths_error': "--selftest-paths: unknown matrix path(s) ['nope']: choose from f16, fp8, bf8, i8, mxfp8, "
                      "mxfp6, mxfp4, f32, f64 or 'all'",
 'agent_paths_empty': "--selftest-paths: name at least one path, or 'all'",
 'main_valu_error': "unknown vector-ALU group(s) ['nope']: choose from fma32, fma64, pkfma16, pkfma32, addmul32, "
                    "int32, int64, bits, dot, cvt, xlane, approx, regs or 'all'",
 'agent_valu_error': "--selftest-valu: unknown vector-ALU group(s) ['nope']: choose from fma32, fma64, pkfma16, "
                     "pkfma32, addmul32, int32, int64, bits, dot, cvt, xlane, approx, regs or 'all'",
 'agent_valu_empty': "--selftest-valu: name at least one group, or 'all'",
 'main_scalar_error': "unknown scalar group(s) ['nope']: choose from add, mul, shift, logic, bits, cmp, vcc, smem, "
                      "sregs or 'all'",
 'agent_scalar_error': "--selftest-scalar: unknown scalar group(s) ['nope']: choose from add, mul, shift, logic, "
                       "bits, cmp, vcc, smem, sregs or 'all'",
 'agent_scalar_empty': "--selftest-scalar: name at least one group, or 'all'",
 'agent_defaults': [[], [], []],
 'metrics': ["# HELP nanogpu_selftest_last_run_timestamp_seconds when the device's last deep self-test ended",
             '# TYPE nanogpu_selftest_last_run_timestamp_seconds gauge',
             'nanogpu_selftest_last_run_timestamp_seconds{device="0"} 0.0',
             '# HELP nanogpu_selftest_cus_checked CUs whose MFMA pipes and LDS the last deep self-test checked',
             '# TYPE nanogpu_selftest_cus_checked gauge', 'nanogpu_selftest_cus_checked{device="0"} 256',
             '# HELP nanogpu_selftest_cus_failed CUs that failed the last deep self-test',
             '# TYPE nanogpu_selftest_cus_failed gauge', 'nanogpu_selftest_cus_failed{device="0"} 2',
             '# HELP nanogpu_selftest_cus_uncovered CUs the last deep self-test was meant to reach and did not',
             '# TYPE nanogpu_selftest_cus_uncovered gauge', 'nanogpu_selftest_cus_uncovered{device="0"} 0',
             '# HELP nanogpu_selftest_hbm_bytes_checked HBM bytes the last deep self-test pattern-checked',
             '# TYPE nanogpu_selftest_hbm_bytes_checked gauge',
             'nanogpu_selftest_hbm_bytes_checked{device="0"} 1073741824',
             '# HELP nanogpu_selftest_hbm_errors 16-byte HBM elements the last deep self-test read back wrong',
             '# TYPE nanogpu_selftest_hbm_errors gauge', 'nanogpu_selftest_hbm_errors{device="0"} 2',
             "# HELP nanogpu_selftest_seconds duration of the device's last deep self-test",
             '# TYPE nanogpu_selftest_seconds gauge', 'nanogpu_selftest_seconds{device="0"} 0',
             '# HELP nanogpu_selftest_runs_total deep self-tests run, by result',
             '# TYPE nanogpu_selftest_runs_total counter', 'nanogpu_selftest_runs_total{device="0",result="fail"} 1',
             '# HELP nanogpu_selftest_paths_checked matrix paths the last deep self-test ran on every CU',
             '# TYPE nanogpu_selftest_paths_checked gauge', 'nanogpu_selftest_paths_checked{device="0"} 9',
             '# HELP nanogpu_selftest_path_cus_failed CUs that failed the matrix path in the last deep self-test',
             '# TYPE nanogpu_selftest_path_cus_failed gauge',
             'nanogpu_selftest_path_cus_failed{device="0",path="f16"} 0',
             'nanogpu_selftest_path_cus_failed{device="0",path="fp8"} 1',
             'nanogpu_selftest_path_cus_failed{device="0",path="bf8"} 0',
             'nanogpu_selftest_path_cus_failed{device="0",path="i8"} 0',
             'nanogpu_selftest_path_cus_failed{device="0",path="mxfp8"} 0',
             'nanogpu_selftest_path_cus_failed{device="0",path="mxfp6"} 0',
             'nanogpu_selftest_path_cus_failed{device="0",path="mxfp4"} 0',
             'nanogpu_selftest_path_cus_failed{device="0",path="f32"} 0',
             'nanogpu_selftest_path_cus_failed{device="0",path="f64"} 0',
             '# HELP nanogpu_selftest_valu_checked vector-ALU groups (with approx and regs) the last deep self-test '
             'ran on every CU',
             '# TYPE nanogpu_selftest_valu_checked gauge', 'nanogpu_selftest_valu_checked{device="0"} 13',
             '# HELP nanogpu_selftest_scalar_checked scalar groups (with smem and sregs) the last deep self-test ran '
             'on every CU',
             '# TYPE nanogpu_selftest_scalar_checked gauge', 'nanogpu_selftest_scalar_checked{device="0"} 9']}
