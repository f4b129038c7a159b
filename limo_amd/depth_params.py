"""Reader of mono_lidar_fusion_parameters.yaml (the flat `key: value  # comment` form the reference application loads)
into a limo_depth_params.  The same reader in C++: limo_amd/kba/depth_params_yaml.hpp."""
import ctypes as C

from . import _ffi

# the file's own spellings of two keys
FILE_SPELLINGS = {"pixelarea_search_witdh": "pixelarea_search_width", "histogram_segmentation_bin_witdh": "histogram_segmentation_bin_width"}
NOT_IN_FILE = ("ransac_seed", "neighbors_count_min")  # ours: the RANSAC seed; the rectangle search's minimum count (the file has
# a minimum for the radius search only, radiusSearch_count_min)


def _parse_int(text):
    return int(text, 10)  # "1.5" for an integer key is an error, as in the C++ reader


def load_depth_params(path, params=None):
    """Defaults (limo_depth_default_params, or `params`) overridden by every key of the file.  An unknown key or a value
    that does not parse raises ValueError naming the line; keys absent from the file keep their defaults."""
    if params is None:
        params = _ffi.DepthParams()
        _ffi.load().limo_depth_default_params(C.byref(params))
    types = {name: typ for name, typ in _ffi.DepthParams._fields_ if name not in NOT_IN_FILE}
    with open(path) as fh:
        for no, raw in enumerate(fh, 1):
            line = raw.split("#", 1)[0].strip()
            if not line or (no == 1 and raw.startswith("%YAML")):
                continue
            key, sep, value = line.partition(":")
            key, value = key.strip(), value.strip()
            field = FILE_SPELLINGS.get(key, key)
            if not sep or field not in types or key in FILE_SPELLINGS.values():
                raise ValueError("%s:%d: unknown key '%s'" % (path, no, key))
            try:
                setattr(params, field, float(value) if types[field] is C.c_double else _parse_int(value))
            except ValueError:
                raise ValueError("%s:%d: cannot read '%s' as a value of %s" % (path, no, value, key)) from None
    return params
