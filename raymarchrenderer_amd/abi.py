"""ctypes mirror of include/rmr.h and include/rmr_tables.h (data layout only).

Every struct here must match the C declaration byte for byte; tests/test_abi.py checks the sizes
against the values the shared library reports.
"""
import ctypes as C

RMR_MAX_VARS = 16
RMR_MAX_PRIMS = 4096
RMR_MAX_OPS = 8192
RMR_MAX_CONSTS = 8192
RMR_MAX_MATERIALS = 256

RMR_VARIANT_RM1 = 1
RMR_VARIANT_RM2 = 2
RMR_VARIANT_RM3 = 3
VARIANTS = {"rm1": RMR_VARIANT_RM1, "rm2": RMR_VARIANT_RM2, "rm3": RMR_VARIANT_RM3}

RMR_PRIM_SPHERE = 1
RMR_PRIM_BOX = 2
RMR_PRIM_PROGRAM = 3
RMR_PRIM_MANDELBULB = 4

RMR_OPND_NONE = -1000000
RMR_OPND_P = -1
RMR_OPND_CONST0 = -2


def opnd_const(k):
    return RMR_OPND_CONST0 - k


# opcodes (rmr_opcode)
OP = {}
_obj = ["GET_X", "GET_Y", "GET_Z", "ADD", "SUB", "MUL", "DIV", "SIN", "COS", "MAP_SPHERE",
        "MAP_BOX", "UNION", "SUBTRACT", "INTERSECT", "DOMAIN_REPEAT", "MAP_MANDELBULB"]
for i, n in enumerate(_obj):
    OP[n] = 1 + i
_mat = ["M_FACING", "M_INSIDE", "M_ADD", "M_SUB", "M_MUL", "M_DIV", "M_MIX", "M_DIFFUSE",
        "M_GLOSSY", "M_REFRACTION", "M_VOLUME", "M_EMISSION"]
for i, n in enumerate(_mat):
    OP[n] = 32 + i
for i, n in enumerate(["V2_DIFFUSE", "V2_GLOSSY", "V2_FRESNEL", "V2_MIX"]):
    OP[n] = 64 + i

RMR_OK = 0
ERRORS = {-1: "RMR_E_INVALID", -2: "RMR_E_HIP", -3: "RMR_E_SCENE", -4: "RMR_E_IO",
          -5: "RMR_E_STATE", -6: "RMR_E_NOMEM", -7: "RMR_E_UNSUPPORTED"}


class Prim(C.Structure):
    _fields_ = [("type", C.c_int32), ("mat_id", C.c_float), ("prog_begin", C.c_int32),
                ("prog_end", C.c_int32), ("c", C.c_float * 3), ("dist_var", C.c_int32),
                ("r", C.c_float * 3), ("n_vars", C.c_int32)]


class Op(C.Structure):
    _fields_ = [("code", C.c_int32), ("inp", C.c_int32 * 7), ("out", C.c_int32 * 4)]


class Material(C.Structure):
    _fields_ = [("defined", C.c_int32), ("prog_begin", C.c_int32), ("prog_end", C.c_int32),
                ("n_vars", C.c_int32), ("color_var", C.c_int32), ("dir_var", C.c_int32),
                ("inside_var", C.c_int32), ("hit_var", C.c_int32)]


class Spectral(C.Structure):
    _fields_ = [("defined", C.c_int32), ("min_wave", C.c_uint32), ("max_wave", C.c_uint32),
                ("power", C.c_float), ("terminates", C.c_int32), ("pad", C.c_int32 * 3)]


class RM2Consts(C.Structure):
    _fields_ = [("albedo", (C.c_float * 3) * RMR_MAX_MATERIALS), ("light_pos", C.c_float * 3),
                ("light_power", C.c_float), ("node_mat_id", C.c_int32), ("pad", C.c_int32 * 3)]


class Scene(C.Structure):
    _fields_ = [("variant", C.c_int32),
                ("n_prims", C.c_int32), ("prims", C.POINTER(Prim)),
                ("n_ops", C.c_int32), ("ops", C.POINTER(Op)),
                ("n_consts", C.c_int32), ("consts", C.POINTER(C.c_float)),
                ("n_materials", C.c_int32), ("materials", C.POINTER(Material)),
                ("spectral", C.POINTER(Spectral)),
                ("spectral_sky", Spectral),
                ("v2_prog_begin", C.c_int32), ("v2_prog_end", C.c_int32), ("v2_n_slots", C.c_int32),
                ("rm2", C.POINTER(RM2Consts)),
                ("sky", C.c_float * 3)]


class Params(C.Structure):
    _fields_ = [("max_dist", C.c_float), ("max_steps", C.c_int32), ("max_bounces", C.c_int32),
                ("step_multiply", C.c_float), ("separate_channels", C.c_int32),
                ("use_env_tex", C.c_int32)]


def default_params(**kw):
    """Graphics::Render's uniform constants (Graphics.cpp:326-340)."""
    p = Params(1000.0, 512, 16, 0.5, 0, 0)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


class Stats(C.Structure):
    _fields_ = [("map_evals", C.c_uint64), ("samples", C.c_uint64), ("trace_launches", C.c_uint64),
                ("trace_ms", C.c_double), ("fold_ms", C.c_double), ("flops_per_map", C.c_double),
                ("map_iters", C.c_uint64), ("shade_batches", C.c_uint64), ("jit_launches", C.c_uint64)]


class DenoiseParams(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("normal_pow2", C.c_int32), ("sigma_z", C.c_float),
                ("sigma_c", C.c_float)]


def default_denoise_params(**kw):
    """rmr_default_denoise_params' values (rmr.h), with overrides."""
    p = DenoiseParams(5, 5, 0.02, 0.0)
    for k, v in kw.items():
        if k not in ("iterations", "normal_pow2", "sigma_z", "sigma_c"):
            raise TypeError("unknown denoise parameter %r" % k)
        setattr(p, k, v)
    return p


DENOISE_FIELDS = ("iterations", "normal_pow2", "sigma_z", "sigma_c")


class VarianceParams(C.Structure):
    _fields_ = [("sigma_l", C.c_float), ("var_radius", C.c_int32)]


VARIANCE_FIELDS = ("sigma_l", "var_radius")


def default_variance_params(**kw):
    """rmr_default_variance_params' values (rmr.h), with overrides."""
    p = VarianceParams(4.0, 3)
    for k, v in kw.items():
        if k not in VARIANCE_FIELDS:
            raise TypeError("unknown variance parameter %r" % k)
        setattr(p, k, v)
    return p


class TemporalParams(C.Structure):
    _fields_ = [("max_history", C.c_float), ("sigma_z", C.c_float), ("normal_pow2", C.c_int32)]


TEMPORAL_FIELDS = ("max_history", "sigma_z", "normal_pow2")


def default_temporal_params(**kw):
    """rmr_default_temporal_params' values (rmr.h), with overrides."""
    p = TemporalParams(64.0, 0.02, 5)
    for k, v in kw.items():
        if k not in TEMPORAL_FIELDS:
            raise TypeError("unknown temporal parameter %r" % k)
        setattr(p, k, v)
    return p


class BloomParams(C.Structure):
    _fields_ = [("levels", C.c_int32), ("threshold", C.c_float), ("clamp", C.c_float), ("scatter", C.c_float),
                ("intensity", C.c_float), ("reserved", C.c_int32 * 3)]


BLOOM_FIELDS = ("levels", "threshold", "clamp", "scatter", "intensity")


def default_bloom_params(**kw):
    """rmr_default_bloom_params' values (rmr.h), with overrides."""
    p = BloomParams(5, 1.0, 0.0, 0.7, 0.2)
    for k, v in kw.items():
        if k not in BLOOM_FIELDS:
            raise TypeError("unknown bloom parameter %r" % k)
        setattr(p, k, v)
    return p


class TonemapParams(C.Structure):
    _fields_ = [("curve", C.c_int32), ("auto_exposure", C.c_int32), ("exposure_ev", C.c_float), ("key", C.c_float),
                ("low_pct", C.c_float), ("high_pct", C.c_float), ("adapt", C.c_float), ("white", C.c_float)]


TONEMAP_FIELDS = ("curve", "auto_exposure", "exposure_ev", "key", "low_pct", "high_pct", "adapt", "white")
# the curves of the tone-mapping stage (rmr.h)
TONE_LINEAR = 0
TONE_REINHARD = 1
TONE_ACES = 2
TONE_CURVES = {"linear": TONE_LINEAR, "reinhard": TONE_REINHARD, "aces": TONE_ACES}


def default_tonemap_params(**kw):
    """rmr_default_tonemap_params' values (rmr.h), with overrides."""
    p = TonemapParams(TONE_ACES, 0, 0.0, 0.18, 0.10, 0.90, 1.0, 4.0)
    for k, v in kw.items():
        if k not in TONEMAP_FIELDS:
            raise TypeError("unknown tonemap parameter %r" % k)
        setattr(p, k, v)
    return p


class AdaptiveParams(C.Structure):
    _fields_ = [("threshold", C.c_float), ("offset", C.c_float), ("min_samples", C.c_uint32),
                ("pass_samples", C.c_uint32), ("max_samples", C.c_uint32), ("block_tiles", C.c_int32)]


class AdaptiveResult(C.Structure):
    _fields_ = [("passes", C.c_uint32), ("tiles_open", C.c_uint32), ("samples", C.c_uint64),
                ("max_error", C.c_float)]


ADAPTIVE_FIELDS = ("threshold", "offset", "min_samples", "pass_samples", "max_samples", "block_tiles")


def default_adaptive_params(**kw):
    """rmr_default_adaptive_params' values (rmr.h), with overrides; max_samples has no default (0)."""
    p = AdaptiveParams(0.1, 1e-4, 16, 16, 0, 2)
    for k, v in kw.items():
        if k not in ADAPTIVE_FIELDS:
            raise TypeError("unknown adaptive parameter %r" % k)
        setattr(p, k, v)
    return p


# camera models (rmr.h rmr_camera_model) and caller-supplied rays (rmr_ray)
CAMERA_VIEW = 0
CAMERA_THIN_LENS = 1
CAMERA_EQUIRECT = 2
CAMERA_ORTHO = 3
CAMERA_MODELS = {"view": CAMERA_VIEW, "thinlens": CAMERA_THIN_LENS, "equirect": CAMERA_EQUIRECT, "ortho": CAMERA_ORTHO}
CAMERA_FIELDS = ("aperture", "focus", "width", "height")


class CameraModel(C.Structure):
    _fields_ = [("model", C.c_int32), ("aperture", C.c_float), ("focus", C.c_float), ("width", C.c_float),
                ("height", C.c_float)]


def default_camera_model(model=CAMERA_VIEW, **kw):
    """rmr_default_camera_model's values (rmr.h) for `model` (abi.CAMERA_* or its name), with overrides."""
    if isinstance(model, str):
        if model not in CAMERA_MODELS:
            raise ValueError("unknown camera model %r (view, thinlens, equirect, ortho)" % model)
        model = CAMERA_MODELS[model]
    m = CameraModel(int(model), 0.0, 1.0, 1.0, 1.0)
    for k, v in kw.items():
        if k not in CAMERA_FIELDS:
            raise TypeError("unknown camera model field %r" % k)
        setattr(m, k, v)
    return m


class Ray(C.Structure):
    _fields_ = [("o", C.c_float * 3), ("time", C.c_float), ("d", C.c_float * 3), ("rc", C.c_float),
                ("gx", C.c_int32), ("gy", C.c_int32)]


# rmr_ray as a numpy structured dtype (Renderer.camera_rays / trace_rays), byte for byte the C struct
RAY_DTYPE = [("o", "<f4", (3,)), ("time", "<f4"), ("d", "<f4", (3,)), ("rc", "<f4"), ("gx", "<i4"), ("gy", "<i4")]


# rmr_hit (rmr_cast_rays): the guide planes' HIT and NORMAL of one ray, 32 bytes
class Hit(C.Structure):
    _fields_ = [("pos", C.c_float * 3), ("t", C.c_float), ("n", C.c_float * 3), ("id", C.c_float)]


HIT_DTYPE = [("pos", "<f4", (3,)), ("t", "<f4"), ("n", "<f4", (3,)), ("id", "<f4")]
CAST_NORMALS = 1

# guide planes and output sources (rmr.h)
GUIDE_RAY = 0
GUIDE_HIT = 1
GUIDE_NORMAL = 2
GUIDE_PLANES = {"ray": GUIDE_RAY, "hit": GUIDE_HIT, "normal": GUIDE_NORMAL}
OUTPUT_ACCUM = 0
OUTPUT_DENOISED = 1
OUTPUT_TEMPORAL = 2
OUTPUT_TONEMAPPED = 3
OUTPUT_BLOOM = 4
OUTPUT_SOURCES = {"accum": OUTPUT_ACCUM, "denoised": OUTPUT_DENOISED, "temporal": OUTPUT_TEMPORAL,
                  "tonemapped": OUTPUT_TONEMAPPED, "bloom": OUTPUT_BLOOM}
# sampled AOVs (rmr.h rmr_render_aov): the raw state planes and the resolved planes
AOV_STATS = 0
AOV_NORMAL = 1
AOV_POSITION = 2
AOV_IDS01 = 3
AOV_IDS23 = 4
AOV_PLANES = {"stats": AOV_STATS, "normal": AOV_NORMAL, "position": AOV_POSITION, "ids01": AOV_IDS01, "ids23": AOV_IDS23}
AOV_R_DEPTH = 0
AOV_R_NORMAL = 1
AOV_R_POSITION = 2
AOV_R_IDS01 = 3
AOV_R_IDS23 = 4
AOV_RESOLVED = {"depth": AOV_R_DEPTH, "normal": AOV_R_NORMAL, "position": AOV_R_POSITION, "ids01": AOV_R_IDS01,
                "ids23": AOV_R_IDS23}


# SDF volume sampling and surface-nets extraction (rmr.h rmr_sample_volume / rmr_extract_mesh)
class VolumeDesc(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("spacing", C.c_float), ("n", C.c_int32 * 3)]


class MeshParams(C.Structure):
    _fields_ = [("iso", C.c_float), ("flags", C.c_int32)]


class MeshInfo(C.Structure):
    _fields_ = [("n_vertices", C.c_uint64), ("n_quads", C.c_uint64)]


def volume_desc(origin, spacing, shape):
    """rmr_volume_desc of a lattice: origin (x, y, z), spacing, shape (nx, ny, nz) points."""
    o, n = [float(v) for v in origin], [int(v) for v in shape]
    if len(o) != 3 or len(n) != 3:
        raise ValueError("a lattice has an origin of 3 coordinates and a shape of 3 point counts")
    return VolumeDesc((C.c_float * 3)(*o), float(spacing), (C.c_int32 * 3)(*n))


MESH_NORMALS = 1
MESH_IDS = 2
MESH_BUF_VERTICES = 0
MESH_BUF_NORMALS = 1
MESH_BUF_IDS = 2
MESH_BUF_QUADS = 3


# light baking at surface points and mesh vertices (rmr.h rmr_bake_points)
BAKE_RADIANCE = 1
BAKE_AO = 2
MESH_BAKE_RGBA = 0
MESH_BAKE_AO = 1


class BakeParams(C.Structure):
    _fields_ = [("flags", C.c_int32), ("bias", C.c_float), ("ao_distance", C.c_float), ("origin_extent", C.c_float),
                ("first_index", C.c_uint64)]


def bake_params(radiance=True, ao=False, bias=0.002, ao_distance=float("inf"), first_index=0, origin_extent=0.0):
    """rmr_bake_params (the defaults are rmr_default_bake_params')."""
    return BakeParams((BAKE_RADIANCE if radiance else 0) | (BAKE_AO if ao else 0), float(bias), float(ao_distance),
                      float(origin_extent), int(first_index))


# irradiance probes (rmr.h rmr_bake_probes)
PROBE_FLOATS = 28
# a probe's visibility map (rmr.h rmr_bake_probe_visibility): 8 x 8 texels of (m1, m2)
PROBE_VIS_RES = 8
PROBE_VIS_TEXELS = 64
PROBE_VIS_FLOATS = 128


class ProbeParams(C.Structure):
    _fields_ = [("clearance", C.c_float), ("origin_extent", C.c_float), ("first_index", C.c_uint64)]


def probe_params(clearance=0.0, first_index=0, origin_extent=0.0):
    """rmr_probe_params (the defaults are rmr_default_probe_params')."""
    return ProbeParams(float(clearance), float(origin_extent), int(first_index))


# variance planes of the variance-guided denoiser (rmr.h)
VARIANCE_SEED = 0
VARIANCE_FILTERED = 1
VARIANCE_PLANES = {"seed": VARIANCE_SEED, "filtered": VARIANCE_FILTERED}
# rmr_set_culling flags (rmr.h)
CULL_ESCAPE = 1
CULL_NPC = 2
CULL_APPROX = 4
CULL_EYE = 8
CULL_ALL = CULL_ESCAPE | CULL_NPC | CULL_APPROX | CULL_EYE
# rmr_set_instrument flags (rmr.h)
INSTR_COUNT_FLOPS = 1
