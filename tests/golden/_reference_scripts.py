"""What make_golden_truth.py and make_golden_eval.py share: loading a script of the reference with stand-ins for the modules it
imports but the fixtures do not need (GDAL, the reference's ``data`` package), a GDAL driver that records what the script writes,
and an ``.npz`` writer whose bytes depend on the arrays alone (``np.savez`` stamps every member with the current time).

The reference's checkout is named by the environment variable ``BGNN_REFERENCE`` or by the first command-line argument."""
import importlib.util
import io
import logging
import os
import sys
import types
import zipfile

import numpy as np


def reference_root():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("BGNN_REFERENCE")
    if not root or not os.path.isdir(os.path.join(root, "scripts")):
        raise SystemExit("usage: BGNN_REFERENCE=<reference checkout> python " + sys.argv[0] + "   (or the checkout as first argument)")
    return root


class RecordedBand:
    def __init__(self):
        self.array = None
        self.description = None
        self.nodata = None

    def WriteArray(self, a):
        self.array = np.array(a, copy=True)

    def SetDescription(self, d):
        self.description = d

    def SetNoDataValue(self, v):
        self.nodata = v


class RecordedDataset:
    def __init__(self, path, width, height, count, dtype, options):
        self.path, self.width, self.height, self.dtype, self.options = path, width, height, dtype, options
        self.bands = [RecordedBand() for _ in range(count)]
        self.geotransform = None
        self.projection = None

    def SetGeoTransform(self, t):
        self.geotransform = tuple(t)

    def SetProjection(self, p):
        self.projection = p

    def GetRasterBand(self, i):
        return self.bands[i - 1]

    def FlushCache(self):
        pass


class RecordingDriver:
    """``gdal.GetDriverByName(...)``: keeps every dataset the script creates."""

    def __init__(self):
        self.datasets = []

    def Create(self, path, width, height, count, dtype, options=None):
        ds = RecordedDataset(path, width, height, count, dtype, options)
        self.datasets.append(ds)
        return ds


def load_reference_script(name):
    """``scripts/<name>.py`` of the reference as a module, with ``osgeo.gdal`` and ``data`` replaced.  Returns the module and the
    recording driver its ``gdal.GetDriverByName`` hands out."""
    driver = RecordingDriver()
    gdal = types.ModuleType("osgeo.gdal")
    gdal.GDT_Float32 = 6
    gdal.GetDriverByName = lambda _name: driver
    osgeo = types.ModuleType("osgeo")
    osgeo.gdal = gdal
    data = types.ModuleType("data")
    data.BathymetricLoader = object
    sys.modules.update({"osgeo": osgeo, "osgeo.gdal": gdal, "data": data})
    path = os.path.join(reference_root(), "scripts", name + ".py")
    spec = importlib.util.spec_from_file_location("reference_" + name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    logging.disable(logging.CRITICAL)
    return mod, driver


def save_npz(path, arrays):
    """A compressed ``.npz`` that ``np.load`` reads, with a fixed member order and time stamp: equal arrays give equal bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())
    return os.path.getsize(path)
