"""The files and cases of the whole-file RGBA tests (test_decode_rgba.py, test_rgba_mode.py, test_hip_codec_rgba.py) and of
tests/golden/make_rgba_golden.py, which records the SHA-256 of every case's expected frame in tests/golden/rgba/rgba.json.

Expected frame of a case = rgba_model applied to libopenjp2's component samples (OpjReplay.decode_comps), written into the
R, G, B, A samples of an After Effects frame whose every byte holds FILL beforehand."""
from __future__ import annotations

import hashlib
import os

import numpy as np

import rgba_model as rm
from conftest import GOLDEN_DIR
from j2k_amd import api, synth

FILL = 0x5A

FILES = {
    "j1": "j1_64x48_rgb8_srgb.jp2", "j2": "j2_64x48_grey8.jp2", "j3": "j3_64x48_rgba8_srgb_alpha.jp2", "j4": "j4_64x48_rgb16_icc.jp2",
    "j5": "j5_64x48_rgb8_sycc_97.jp2", "j6": "j6_40x30_greya8.jp2", "j7": "j7_40x30_cmyk8.jp2", "j8": "j8_40x30_rgb8_unspecified.jp2",
    "j9": "j9_40x30_rgba16_icc_alpha.jp2", "jr1": "jr1_300x200_rgba8_jp2_srgb_alpha_r30_8.jp2", "g3": "g3_300x200_rgb8_53_rct.j2k",
    "u1": os.path.join("ext", "u1_300x200_ycc420_8_53.j2k"), "u6": os.path.join("ext", "u6_200x150_rgb8_53_offset.j2k"),
    "k1": os.path.join("rgba", "k1_37x21_sycc420_8_53.jp2"), "k2": os.path.join("rgba", "k2_65x33_sycc422_10_97.jp2"),
    "k3": os.path.join("rgba", "k3_41x23_sycc420_8_53_origin.jp2"), "k4": os.path.join("rgba", "k4_130x70_sycc420_8_53_tile64.jp2"),
}
# the mode each file must be classified as (None: J2K_HIP_ERR_UNSUPPORTED); "pal" is crafted from j2 at run time
MODES = {"j1": rm.RGB, "j2": rm.GREY, "j3": rm.RGB, "j4": rm.RGB, "j5": rm.SYCC, "j6": rm.GREY, "j7": None, "j8": rm.RGB, "j9": rm.RGB,
         "jr1": rm.RGB, "g3": rm.RGB, "u1": rm.RGB, "u6": rm.RGB, "k1": rm.SYCC, "k2": rm.SYCC, "k3": rm.SYCC, "k4": rm.SYCC, "pal": rm.PALETTE}
PAL_COLUMNS = (1, 2, 0)  # the cmap of "pal": channel i names palette column PAL_COLUMNS[i]
_cache = {}


def load(name: str) -> bytes:
    if name not in _cache:
        if name == "pal":
            from test_read_fallback import _with_palette
            _cache[name] = _with_palette(load("j2"), 200, 3, PAL_COLUMNS)[0]
        else:
            with open(os.path.join(GOLDEN_DIR, FILES[name]), "rb") as f:
                _cache[name] = f.read()
    return _cache[name]


def palette(name: str):
    """(lut, lut_rgb) of a palettised file from its header: R / G / B take the column c whose lut_column[c] is 0 / 1 / 2."""
    fi = api.read_info(load(name))
    if not fi["lut_size"]:
        return None, (0, 1, 2)
    cols = list(fi["lut_column"][:fi["lut_channels"]])
    return np.array(fi["lut"], dtype=np.uint8), tuple(cols.index(k) if k in cols[:3] else k for k in range(3))


def _case(file, bits, subsample=1, region=None, demote=False, alpha=True, device=False, pad=0):
    cid = f"{file}-{bits}" + (f"-s{subsample}" if subsample > 1 else "") + ("-r" + "_".join(map(str, region)) if region else "") + \
          ("-demote" if demote else "") + ("" if alpha else "-noalpha") + (f"-pad{pad}" if pad else "")
    return dict(id=cid, file=file, bits=bits, subsample=subsample, region=region, demote=demote, alpha=alpha, device=device, pad=pad)


K4_WINDOWS = [(0, 0, 130, 70), (63, 31, 5, 7), (61, 59, 9, 9), (62, 62, 4, 4), (65, 65, 1, 1), (1, 1, 129, 69), (127, 3, 3, 66)]


def cases():
    out = []
    for f in MODES:
        if MODES[f] is None:
            continue
        out += [_case(f, 8), _case(f, 16), _case(f, 16, demote=True)]
    for f in ("k1", "k2"):
        out += [_case(f, 8, subsample=2), _case(f, 16, subsample=2, demote=True)]
    out += [_case("k1", 8, alpha=False), _case("k1", 16, alpha=False, pad=6), _case("k3", 8, pad=4), _case("j6", 16, pad=8, demote=True)]
    for w in K4_WINDOWS:
        out += [_case("k4", 8, region=w), _case("k4", 16, region=w, demote=True)]
    return out


def device_variant(case):
    """The same case through a device copy of the frame: the same expected bytes."""
    return dict(case, device=True)


def image_size(case):
    """Width and height of the frame: the image at the case's subsample, or its window."""
    if case["region"]:
        return case["region"][2], case["region"][3]
    i = api.read_info(load(case["file"]))
    red = case["subsample"].bit_length() - 1
    return -(-i["width"] >> red), -(-i["height"] >> red)


def blank_frame(case):
    """(frame, layout): an A,R,G,B frame of the case's size and sample type, every byte FILL."""
    w, h = image_size(case)
    frame, lay = synth.ae_frame(np.zeros((4, h, w), dtype=np.int32), case["bits"], row_pad_bytes=case["pad"])
    frame[:] = FILL
    return frame, lay


def expected_from_comps(case, comps):
    """The expected frame from per-component samples (OpjReplay.decode_comps' dicts, or the like) of the whole image at the
    case's subsample."""
    w, h = image_size(case)
    org = tuple(case["region"][:2]) if case["region"] else (0, 0)
    lut, lut_rgb = palette(case["file"])
    planes = rm.file_rgba(MODES[case["file"]], comps, w, h, case["bits"], case["bits"], org, lut, lut_rgb, case["demote"])
    frame, lay = blank_frame(case)
    return rm.into_ae_frame(frame, lay, planes, case["alpha"])


def expected_from_opj(opj, case):
    return expected_from_comps(case, opj.decode_comps(load(case["file"]), reduce=case["subsample"].bit_length() - 1))


def sha(frame: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(frame).tobytes()).hexdigest()
