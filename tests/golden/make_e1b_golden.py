"""Generate tests/golden/e1b_codes.npz from the reference's Galileo code listing.

GALILEO/E1/include/galileo-primary-code.txt is the ICD annex C listing the
reference ships as data: section C.7 holds the 50 E1-B primary codes, each as
"E1B Code No <n>" followed by 1023 hex digits (4092 chips) over several lines.
The digits become chips the way GALILEO/E1/include/readE1Bcode.sci's tail does:
every hex digit is four bits, most significant first (dec2bin(hex2dec(.), 4)),
and E1Bcode = 2 * bit - 1, so bit 1 is chip +1 and bit 0 is chip -1.

Stored: codes (3, 4092) int8, the chips of E1B PRN 11, 12 and 19, and prns.
The parse is trusted only after PRN 1 is seen to start with hex F5D71013.

Usage:  python tests/golden/make_e1b_golden.py [reference root]
"""
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LISTING = os.path.join("trunk", "GNSS_SOFTWARE_RECEIVERS", "POSTPROCESSING_SCILAB_RECEIVERS",
                       "GALILEO", "E1", "include", "galileo-primary-code.txt")
PRNS = (11, 12, 19)
N_CHIPS = 4092


def e1b_hex(path):
    """{prn: its 1023 hex digits} of section C.7."""
    txt = open(path, encoding="latin-1").read()
    start = txt.index("Primary Codes for the E1-B Component")
    end = txt.index("Primary Codes for the E1-C Component")
    out = {}
    parts = re.split(r"E1B Code No\s+(\d+)", txt[start:end])
    for no, body in zip(parts[1::2], parts[2::2]):
        digits = "".join(ln.strip() for ln in body.splitlines()
                         if re.fullmatch(r"[0-9A-F]+", ln.strip()))
        out[int(no)] = digits
    return out


def chips(hexdigits):
    bits = np.array([int(b) for h in hexdigits for b in format(int(h, 16), "04b")], np.int8)
    return (2 * bits - 1).astype(np.int8)


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    codes = e1b_hex(os.path.join(root, LISTING))
    assert sorted(codes) == list(range(1, 51)), sorted(codes)
    assert all(len(v) == N_CHIPS // 4 for v in codes.values()), {k: len(v) for k, v in codes.items()}
    assert codes[1].startswith("F5D71013"), codes[1][:8]
    out = np.stack([chips(codes[p]) for p in PRNS])
    assert out.shape == (len(PRNS), N_CHIPS) and set(np.unique(out)) == {-1, 1}
    np.savez_compressed(os.path.join(HERE, "e1b_codes.npz"), codes=out,
                        prns=np.array(PRNS, np.int32))
    print("e1b_codes.npz", out.shape, out.dtype)


if __name__ == "__main__":
    main()
