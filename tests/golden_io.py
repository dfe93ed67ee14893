"""Reading and writing golden fixtures that are stored in parts.

The reference-mappm vectors are about 3 MB compressed; no committed file is larger than
1 MiB, so they are stored as ``tests/golden/mappm_golden.partN.npz`` (whole arrays,
in key order) and read back as one mapping.
"""
import glob
import io
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PART_BYTES = 768 * 1024  # compressed size at which a new part starts


def _compressed_size(name, array):
    buf = io.BytesIO()
    np.savez_compressed(buf, **{name: array})
    return buf.getbuffer().nbytes


def save_parts(stem, arrays, directory=GOLDEN):
    """Write ``arrays`` (name -> array) as ``<stem>.partN.npz``, each under PART_BYTES;
    returns the paths.  Parts of an earlier call are replaced."""
    for old in glob.glob(os.path.join(directory, f"{stem}.part*.npz")):
        os.remove(old)
    parts, size = [{}], 0
    for name, a in arrays.items():
        n = _compressed_size(name, a)
        if parts[-1] and size + n > PART_BYTES:
            parts.append({})
            size = 0
        parts[-1][name] = a
        size += n
    paths = []
    for i, part in enumerate(parts):
        paths.append(os.path.join(directory, f"{stem}.part{i}.npz"))
        np.savez_compressed(paths[-1], **part)
    return paths


def load_parts(stem, directory=GOLDEN):
    """Every array of ``<stem>.partN.npz`` as one dict (name -> array)."""
    paths = sorted(glob.glob(os.path.join(directory, f"{stem}.part*.npz")))
    if not paths:
        raise FileNotFoundError(f"no {stem}.part*.npz under {directory}")
    out = {}
    for p in paths:
        with np.load(p) as z:
            for name in z.files:
                if name in out:
                    raise ValueError(f"{name} is in more than one part of {stem}")
                out[name] = z[name]
    return out


def load_mappm_golden():
    return load_parts("mappm_golden")
