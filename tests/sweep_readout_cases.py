"""The state-independence cases of include/bmo_sweep_readout.h (not a test file): the registry tests/state_cases.py keeps for include/bmo.h,
under the same rule (DESIGN.md §2 "State independence"), for the header of the through-focus and MTF read-outs of sweeps.

A case is a function without arguments that returns everything its entries write as a dict of arrays; `entries` names the C entries of the
header it reaches.  tests/test_sweep_readout_cases.py holds the union of the `entries` to the header, tests/test_sweep_readout_state_gpu.py
runs the cases.  Every case reads state_cases._PsfSweep: a three-configuration sweep whose middle configuration has no roots (300 and 257
rows in the others), the detector at another pose in each.  What the middle configuration is handed for axes, planes and centres is NaN: a
configuration without rows reads what a single call without rows reads, whatever they hold."""
import os
import re

import numpy as np

import state_cases as sc
from bmo_amd import abi

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bmo_sweep_readout.h")
GROUP = "focus_sweep"  # one child process of the poisoned-pools leg runs them all
CASES = []
K = 3
M_PLANES = sc.M_PLANES  # 17: two chunks of 8 and a plane of the statistics and the geometric MTF, a chunk of 16 and a slot of the stack
mm = 1e-3


def case(*entries):
    def deco(f):
        f.group, f.entries, f.name = GROUP, tuple(entries), f.__name__
        CASES.append(f)
        return f

    return deco


def header_declarations():
    """{entry: parameter count} of the C entries include/bmo_sweep_readout.h declares."""
    text = open(HEADER, encoding="utf-8").read()
    return {name: len(params.split(",")) for name, params in re.findall(r"^int\s+(bmo_[a-z0-9_]+)\(([^)]*)\)\s*;", text, re.M | re.S)}


def _planes(sw):
    """(axes [3, 3], offsets [3, M], displacements [3, M, 3], centres [3, M, 2]): each configuration's own, NaN for the empty one"""
    axes = np.cross(sw.e2, sw.e1)  # the detector's local y
    off = np.linspace(-1 * mm, 1 * mm, M_PLANES)[None, :] * (1 + 0.25 * np.arange(K))[:, None] + 0.01 * mm * np.arange(K)[:, None]
    disp = off[:, :, None] * axes[:, None, :] + 1e-6 * np.arange(K)[:, None, None] * sw.e1[:, None, :]
    cen = np.stack([1e-6 * np.arange(M_PLANES), -2e-6 * np.arange(M_PLANES)], axis=1)[None, :, :] * (1 + np.arange(K))[:, None, None]
    for a in (axes, off, disp, cen):
        a[1] = np.nan
    return axes, off, disp, cen


def _axes(n):
    xs, zs = sc._axes(n)
    ax, az = np.tile(xs, (K, 1)) + 1e-6 * np.arange(K)[:, None], np.tile(zs, (K, 1)) * (1 + 0.1 * np.arange(K))[:, None]
    ax[1], az[1] = np.nan, np.nan
    return ax, az


@case("bmo_psf_focus_stats_sweep")
def psf_focus_stats_sweep():
    with sc._PsfSweep() as sw:
        axes, off, _, _ = _planes(sw)
        return {"stats": abi.psf_focus_stats_sweep(sw.handle, sw.slot, K, sw.pos, sw.e1, sw.e2, axes, off)[0],
                "one_list": abi.psf_focus_stats_sweep(sw.handle, sw.slot, K, sw.pos, sw.e1, sw.e2, np.nan_to_num(axes), off[0])[0]}


@case("bmo_psf_through_focus_sweep")
def psf_through_focus_sweep():
    out = {}
    with sc._PsfSweep() as sw:
        _, _, disp, _ = _planes(sw)
        xs, zs = _axes(5)
        sc._put(out, "field/", ("I", "F"), abi.psf_through_focus_sweep(sw.handle, sw.slot, K, sw.pos, sw.e1, sw.e2, disp, xs, zs, want_field=True)[:2])
        sc._put(out, "plain/", ("I", "F"), abi.psf_through_focus_sweep(sw.handle, sw.slot, K, sw.pos, sw.e1, sw.e2, disp, xs, zs)[:2])
    return out


@case("bmo_psf_geo_otf_sweep")
def psf_geo_otf_sweep():
    out = {}
    with sc._PsfSweep() as sw:
        axes, off, _, cen = _planes(sw)
        names = ("mtf", "otf", "sums")
        sc._put(out, "origin/", names, abi.psf_geo_otf_sweep(sw.handle, sw.slot, K, sw.pos, sw.e1, sw.e2, axes, off, sc.FREQS)[:3])
        sc._put(out, "centers/", names, abi.psf_geo_otf_sweep(sw.handle, sw.slot, K, sw.pos, sw.e1, sw.e2, axes, off, sc.FREQS, centers=cen)[:3])
    return out


@case("bmo_psf_otf_sweep")
def psf_otf_sweep():
    out = {}
    with sc._PsfSweep() as sw:
        _, _, disp, _ = _planes(sw)
        xs, zs = _axes(5)
        names = ("mtf", "otf", "sums", "I")
        sc._put(out, "image/", names, abi.psf_otf_sweep(sw.handle, sw.slot, K, sw.pos, sw.e1, sw.e2, disp, xs, zs, sc.FREQS, want_intensity=True)[:4])
        sc._put(out, "plain/", names, abi.psf_otf_sweep(sw.handle, sw.slot, K, sw.pos, sw.e1, sw.e2, disp, xs, zs, sc.FREQS)[:4])
    return out
