"""ctypes bindings for include/terra.h (libterra_hip.so).  Host glue only -- no arithmetic happens in Python."""
import ctypes as C
import os
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

GEN_GLACIATE, GEN_FORCE_SINE, GEN_NO_WAIT, GEN_CACHE_VALUES, GEN_FUSED, GEN_FAST = 1, 2, 4, 8, 16, 32
ERODE_SERIAL, ERODE_MINZ_IS_MIN, ERODE_SERIAL_WAVE = 1, 2, 4
MGEN_SINE, MGEN_SIMPLEX, MGEN_PERLIN, MGEN_SIMPLEX_GPU, MGEN_DWARP_GPU = range(5)


class TerraError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"terra error {code}: {msg}")
        self.code = code


class Config(C.Structure):  # terra_config
    _fields_ = [("mesh_x", C.c_int32), ("mesh_y", C.c_int32), ("scene_x", C.c_float), ("scene_y", C.c_float), ("scene_z", C.c_float),
                ("mesh_height", C.c_float), ("mesh_scale", C.c_float), ("mesh_seed", C.c_int32), ("mesh_freq_filter", C.c_int32),
                ("mesh_gen_mode", C.c_int32), ("mesh_gen_shape", C.c_int32), ("glaciate", C.c_int32), ("custom_glaciate_exp", C.c_float),
                ("hmap", C.c_float * 14), ("erode_amount", C.c_float), ("water_h_off", C.c_float), ("water_h_off_rel", C.c_float),
                ("relh_adj_tex", C.c_float), ("ocean_wave_height", C.c_float),
                ("start_mag", C.c_float), ("start_freq", C.c_float), ("mag_mult", C.c_float), ("freq_mult", C.c_float)]


_STATE_FLOATS = ("MESH_HEIGHT DX_VAL DY_VAL DX_VAL_INV DY_VAL_INV HALF_DXY dxdy XY_SCENE_SIZE mesh_scale mesh_scale_z_inv "
                 "mesh_height_scale zmax_est zmin zmax water_plane_z glaciate_exp clip_hd1 relh_adj_tex rx ry").split()


class State(C.Structure):  # terra_state
    _fields_ = [("sinTable", (C.c_float * 5) * 90), ("start_eval_sin", C.c_int32)] + [(n, C.c_float) for n in _STATE_FLOATS]


class TileStats(C.Structure):  # terra_tile_stats
    _fields_ = [("sub_zmin", C.c_float * 16), ("sub_zmax", C.c_float * 16), ("mzmin", C.c_float), ("mzmax", C.c_float), ("radius", C.c_float),
                ("wx1", C.c_int32), ("wy1", C.c_int32), ("wx2", C.c_int32), ("wy2", C.c_int32)]


class Landscape(C.Structure):  # terra_landscape
    _fields_ = [("vegetation", C.c_float), ("temperature", C.c_float), ("biome_x_offset", C.c_float), ("mesh_scale_z", C.c_float),
                ("water_is_lava", C.c_int32), ("disable_water", C.c_int32), ("enable_terrain_env", C.c_int32),
                ("grass_density", C.c_uint32), ("num_rnd_grass_blocks", C.c_uint32)]


def make_landscape(vegetation=1.0, temperature=20.0, biome_x_offset=0.0, mesh_scale_z=1.0, water_is_lava=0, disable_water=0,
                   enable_terrain_env=1, grass_density=0, num_rnd_grass_blocks=16):
    """terra_landscape with the reference's defaults."""
    return Landscape(vegetation, temperature, biome_x_offset, mesh_scale_z, water_is_lava, disable_water, enable_terrain_env, grass_density, num_rnd_grass_blocks)


BRUSH_DTYPE = np.dtype({"names": ["x", "y", "radius", "delta", "shape"], "formats": [np.int32, np.int32, np.uint32, np.int32, np.int16], "itemsize": 20})  # terra_hmap_brush
MOD_DTYPE = np.dtype([("x", np.uint16), ("y", np.uint16), ("delta", np.int32)])  # terra_hmap_mod
GRASS_BLOCK_DTYPE = np.dtype([("ix", np.uint32), ("zmin", np.float32), ("zmax", np.float32)])  # terra_grass_block
LINE_HIT_DTYPE = np.dtype([("t", np.float32), ("tile", np.int32), ("xpos", np.int32), ("ypos", np.int32), ("p_int", np.float32, (3,)), ("hit", np.uint32)])  # terra_line_hit
assert LINE_HIT_DTYPE.itemsize == 32
LINE_TREE_HIT_DTYPE = np.dtype([("t", np.float32), ("tile", np.int32), ("xpos", np.int32), ("ypos", np.int32), ("p_int", np.float32, (3,)), ("hit", np.uint32),
                                ("tree", np.int32), ("part", np.uint32)])  # terra_line_tree_hit
assert LINE_TREE_HIT_DTYPE.itemsize == 40
LINE_HIT_NONE, LINE_HIT_MESH, LINE_HIT_TREE = 0, 1, 2  # terra_line_tree_hit.hit
TREE_SPLAT_DTYPE = np.dtype([("x", np.float32), ("y", np.float32), ("radius", np.float32)])  # terra_tree_splat
assert TREE_SPLAT_DTYPE.itemsize == 12
TREE_PLACE_DTYPE = np.dtype([("pos", np.float32, (3,)), ("type", np.int32), ("inst", np.int32), ("height", np.float32), ("width", np.float32),
                             ("rseed1", np.int32), ("rseed2", np.int32), ("cx", np.uint16), ("cy", np.uint16)])  # terra_tree_place
assert TREE_PLACE_DTYPE.itemsize == 40


class TreeParams(C.Structure):  # terra_tree_params
    _fields_ = [("sm_tree_density", C.c_float), ("tree_scale", C.c_float), ("tree_density_thresh", C.c_float), ("tree_type_rand_zone", C.c_float),
                ("tree_mode", C.c_int32), ("force_tree_class", C.c_int32), ("only_pine_palm_trees", C.c_int32), ("rand_gen_index", C.c_int32),
                ("instanced", C.c_int32), ("num_pine_insts", C.c_uint32), ("num_palm_insts", C.c_uint32)]


def make_tree_params(sm_tree_density=1.0, tree_scale=1.0, tree_density_thresh=0.55, tree_type_rand_zone=0.0, tree_mode=1, force_tree_class=-1,
                     only_pine_palm_trees=0, rand_gen_index=0, instanced=0, num_pine_insts=0, num_palm_insts=0):
    """terra_tree_params with the reference's defaults (tree_mode 1: no small trees)."""
    return TreeParams(sm_tree_density, tree_scale, tree_density_thresh, tree_type_rand_zone, tree_mode, force_tree_class, only_pine_palm_trees, rand_gen_index,
                      int(bool(instanced)), num_pine_insts, num_palm_insts)


DECID_PLACE_DTYPE = np.dtype([("pos", np.float32, (3,)), ("zval", np.float32), ("type", np.int32), ("tree_id", np.int32), ("rseed1", np.int32), ("rseed2", np.int32),
                              ("cx", np.uint16), ("cy", np.uint16)])  # terra_decid_place
assert DECID_PLACE_DTYPE.itemsize == 36


class DecidParams(C.Structure):  # terra_decid_params
    _fields_ = [("num_trees", C.c_int32), ("num_shared_trees", C.c_uint32), ("tree_slope_thresh", C.c_float), ("branch_size", C.c_float * 5)]


def make_decid_params(num_trees=0, num_shared_trees=0, tree_slope_thresh=5.0, branch_size=(1.0, 1.0, 1.0, 1.0, 1.0)):
    """terra_decid_params with the reference's defaults (num_trees 0: no generated trees)."""
    return DecidParams(num_trees, num_shared_trees, tree_slope_thresh, (C.c_float * 5)(*branch_size))


SCENERY_PLACE_DTYPE = np.dtype([("pos", np.float32, (3,)), ("radius", np.float32), ("kind", np.int32), ("iv", np.int32, (2,)), ("p", np.float32, (8,)),
                                ("rseed1", np.int32), ("rseed2", np.int32), ("cx", np.uint16), ("cy", np.uint16)])  # terra_scenery_place
assert SCENERY_PLACE_DTYPE.itemsize == 72
SCENERY_KINDS = ("leafy_plant", "plant", "rock_shape", "surface_rock", "voxel_rock", "rock", "log", "stump", "mushroom")  # TERRA_SCENERY_*


class SceneryParams(C.Structure):  # terra_scenery_params
    _fields_ = [("use_voxel_rocks", C.c_int32)]


def make_scenery_params(use_voxel_rocks=2):
    """terra_scenery_params with the reference's default (voxel rocks only when the landscape has no vegetation)."""
    return SceneryParams(use_voxel_rocks)


FLOWER_DTYPE = np.dtype([("pos", np.float32, (3,)), ("normal", np.float32, (3,)), ("radius", np.float32), ("height", np.float32), ("color", np.float32, (4,))])  # terra_flower
assert FLOWER_DTYPE.itemsize == 48
FLOWER_AUX_FIXED = 7  # the aux word's colour field under a fixed flower_color


def flower_aux_fields(aux):
    """the aux words of tiles_place_flowers -> (cx, cy, colour field: 2 + the signed remainder int(1.5*color_val) % 3, or FLOWER_AUX_FIXED)"""
    aux = np.asarray(aux, np.uint32)
    return aux & 1023, (aux >> 10) & 1023, (aux >> 20) & 7


class FlowerParams(C.Structure):  # terra_flower_params
    _fields_ = [("flower_density", C.c_float), ("grass_length", C.c_float), ("grass_width", C.c_float), ("flower_color", C.c_float * 4), ("no_grass", C.c_int32)]


def make_flower_params(flower_density=0.0, grass_length=0.02, grass_width=0.002, flower_color=(0.0, 0.0, 0.0, 0.0), no_grass=0):
    """terra_flower_params with the reference's defaults (flower_density 0: no flowers)."""
    return FlowerParams(flower_density, grass_length, grass_width, (C.c_float * 4)(*flower_color), int(bool(no_grass)))


class View(C.Structure):  # terra_view: pos_dir_up's pos, dir, upv_, cp, sterm, x_sterm, near_, far_, valid
    _fields_ = [("pos", C.c_float * 3), ("dir", C.c_float * 3), ("upv", C.c_float * 3), ("cp", C.c_float * 3), ("sterm", C.c_float), ("x_sterm", C.c_float),
                ("near_", C.c_float), ("far_", C.c_float), ("valid", C.c_int32)]


class GrassViewParams(C.Structure):  # terra_grass_view_params
    _fields_ = [("tt_grass_scale_factor", C.c_float)]


def make_grass_view_params(tt_grass_scale_factor=1.0):
    """terra_grass_view_params with the reference's default."""
    return GrassViewParams(tt_grass_scale_factor)


GRASS_VIEW_LODS = 6      # NUM_GRASS_LODS
GRASS_VIEW_NO_PASS = 255  # the pass byte of a tile that draws nothing


def grass_view_aux_fields(aux):
    """the aux words of tiles_grass_view -> (block index y*dim + x, LOD, bix)"""
    aux = np.asarray(aux, np.uint32)
    return aux & 0xFFFF, (aux >> 16) & 7, aux >> 19


class TerrainViewArgs(C.Structure):  # terra_terrain_view_args
    _fields_ = [("behind_sphere_mult", C.c_float), ("occluder_zmin", C.c_float), ("water_enabled", C.c_int32), ("check_occlusion", C.c_int32), ("reflection_pass", C.c_int32)]


def make_terrain_view_args(behind_sphere_mult=1.0, occluder_zmin=0.0, water_enabled=1, check_occlusion=1, reflection_pass=0):
    """terra_terrain_view_args: behind_sphere_mult from Terra.view_behind_sphere_mult or camera_pdu, occluder_zmin the engine's zmin"""
    return TerrainViewArgs(behind_sphere_mult, occluder_zmin, int(water_enabled), int(check_occlusion), int(reflection_pass))


TERRAIN_VIEW_LODS = 5        # NUM_LODS
TERRAIN_VIEW_NO_CRACK = 255  # the crack byte where there is no present neighbour or the tile is not drawn
TVIEW_ABSENT, TVIEW_TOO_FAR, TVIEW_NOT_VISIBLE, TVIEW_OCCLUDED_BEFORE, TVIEW_OCCLUDED, TVIEW_DRAWN = range(6)  # the low bits of the status byte
TVIEW_STATUS_MASK, TVIEW_WAS_OCCLUDER = 7, 0x80
TVIEW_FLAG_ABSENT, TVIEW_FLAG_NO_OCCLUDER, TVIEW_FLAG_SHADOW_MAPS = 1, 2, 4  # the per-tile flag byte of tiles_terrain_view

TVIEW_NO_REFLECTION = 6      # tiles_reflection_view: the tile was dropped at can_have_reflection
REFLECT_NOT_ASKED, REFLECT_NO_WATER, REFLECT_WALK_NOTHING, REFLECT_HAS_WATER, REFLECT_WALK_FOUND = range(5)  # the reflect byte of tiles_reflection_view


class ReflectionViewArgs(C.Structure):  # terra_reflection_view_args
    _fields_ = [("tv", TerrainViewArgs), ("zmax", C.c_float)]


def make_reflection_view_args(behind_sphere_mult=1.0, zmin=0.0, zmax=0.0, water_enabled=1, check_occlusion=1, reflection_pass=1):
    """terra_reflection_view_args: a terra_terrain_view_args of reflection pass 1 whose occluder_zmin is the engine's zmin, and the engine's zmax"""
    return ReflectionViewArgs(make_terrain_view_args(behind_sphere_mult, zmin, water_enabled, check_occlusion, reflection_pass), zmax)


class WaterViewArgs(C.Structure):  # terra_water_view_args
    _fields_ = [("behind_sphere_mult", C.c_float), ("water_enabled", C.c_int32)]


def make_water_view_args(behind_sphere_mult=1.0, water_enabled=1):
    return WaterViewArgs(behind_sphere_mult, int(water_enabled))


class SmapPlanArgs(C.Structure):  # terra_smap_plan_args
    _fields_ = [("behind_sphere_mult", C.c_float), ("water_enabled", C.c_int32), ("smap_thresh_scale", C.c_float), ("shadow_map_sz", C.c_uint32), ("have_buildings", C.c_int32),
                ("draw_model", C.c_int32), ("b_ext", C.c_float * 3), ("road_len", C.c_float * 2), ("models_z2", C.c_float), ("models_valid", C.c_int32),
                ("sun_pos", C.c_float * 3), ("want_recomp", C.c_int32)]


def make_smap_plan_args(behind_sphere_mult=1.0, water_enabled=1, smap_thresh_scale=1.0, shadow_map_sz=4096, have_buildings=0, draw_model=0, b_ext=(0.0, 0.0, 0.0),
                        road_len=(0.0, 0.0), models_z2=0.0, models_valid=0, sun_pos=(0.0, 0.0, 1.0), want_recomp=0):
    """terra_smap_plan_args: shadow_map_sz 0 means shadow_map_enabled() is false; b_ext / road_len are get_buildings_max_extent() / get_road_max_len()"""
    return SmapPlanArgs(behind_sphere_mult, int(water_enabled), smap_thresh_scale, int(shadow_map_sz), int(have_buildings), int(draw_model), (C.c_float * 3)(*b_ext),
                        (C.c_float * 2)(*road_len), models_z2, int(models_valid), (C.c_float * 3)(*sun_pos), int(want_recomp))


class SmapCastArgs(C.Structure):  # terra_smap_cast_args
    _fields_ = [("water_enabled", C.c_int32), ("decid_trees_only", C.c_int32), ("inc_adj_smap", C.c_int32), ("b_ext", C.c_float * 3), ("road_len", C.c_float * 2)]


def make_smap_cast_args(water_enabled=1, decid_trees_only=0, inc_adj_smap=0, b_ext=(0.0, 0.0, 0.0), road_len=(0.0, 0.0)):
    return SmapCastArgs(int(water_enabled), int(decid_trees_only), int(inc_adj_smap), (C.c_float * 3)(*b_ext), (C.c_float * 2)(*road_len))


SMAP_NONE = 0xFF  # the smap_state byte of a tile without shadow maps
(SMAP_IN_DRAW_DIST, SMAP_VISIBLE, SMAP_BOUNDS_VISIBLE, SMAP_UPDATE, SMAP_CLEARED_FAR, SMAP_CLEARED_WIREFRAME, SMAP_CLEARED_LOD_REDUCE, SMAP_CLEARED_LOD_RAISE, SMAP_ALLOCATED,
 SMAP_RECEIVER, SMAP_USABLE) = (1 << k for k in range(11))  # the plan word of tiles_smap_plan; bits 16-19 lod_level, 20-23 lod_level_reduce
SMAP_TILE_FULLY_IN_CITY = 8  # a bit of the per-tile flags byte
SMAP_CAST_NO_TILE = 1        # the status byte of a render without a receiver


class CloudParams(C.Structure):  # terra_cloud_params
    _fields_ = [("clouds_per_tile", C.c_float), ("cloud_height_offset", C.c_float), ("rgen_seed", C.c_int32)]


def make_cloud_params(clouds_per_tile=0.5, cloud_height_offset=0.0, rgen_seed=1):
    """terra_cloud_params with the reference's defaults"""
    return CloudParams(clouds_per_tile, cloud_height_offset, int(rgen_seed))


class CloudStep(C.Structure):  # terra_cloud_step
    _fields_ = [("wind", C.c_float * 3), ("fticks", C.c_float), ("animate", C.c_int32)]


def make_cloud_step(wind=(0.4, 0.2, 0.0), fticks=1.0, animate=1):
    return CloudStep((C.c_float * 3)(*wind), fticks, int(animate))


class CloudViewArgs(C.Structure):  # terra_cloud_view_args
    _fields_ = [("behind_sphere_mult", C.c_float), ("xlate", C.c_float * 3), ("max_dist", C.c_float)]


def make_cloud_view_args(behind_sphere_mult=1.0, xlate=(0.0, 0.0, 0.0), max_dist=1.0):
    return CloudViewArgs(behind_sphere_mult, (C.c_float * 3)(*xlate), max_dist)


CLOUD_DTYPE = np.dtype([("pos_hash", np.float32), ("pos", np.float32, 3), ("size", np.float32, 3), ("pad", np.uint32)])  # terra_cloud
CLOUD_TILE_DTYPE = np.dtype([("generated", np.uint32), ("flags", np.uint32), ("count", np.uint32), ("num_clouds", np.uint32), ("cur_move_dist", np.float32), ("pad", np.uint32),
                             ("rseed1", np.int64), ("rseed2", np.int64), ("bcube", np.float32, 6), ("range", np.float32, 6)])  # terra_cloud_tile
CLOUD_INST_DTYPE = np.dtype([("tile", np.uint32), ("slot", np.uint32), ("dist_sq", np.float32), ("alpha", np.float32), ("draw_alpha", np.float32), ("drawn", np.uint32)])  # terra_cloud_inst
CLD_OVERFLOW = 1
CLV_NONE, CLV_VFC, CLV_BELOW_ZMIN, CLV_BELOW_WATER, CLV_BELOW_MESH, CLV_LISTED = range(6)  # the stage byte of tiles_cloud_view


class CollideIn(C.Structure):  # terra_collide_in
    _fields_ = [(k, C.c_void_p) for k in ("stats", "trmax", "tile_zmax", "flags", "pine", "pine_counts", "trunk_override", "decid", "decid_counts", "scenery", "scenery_counts",
                                          "radius_override", "tree_data", "br_scale")] + \
               [(k, C.c_uint32) for k in ("pine_capacity", "decid_capacity", "scenery_capacity", "num_tree_data")] + \
               [(k, C.c_int32) for k in ("dxoff", "dyoff", "ptree_xoff2", "ptree_yoff2", "dtree_xoff2", "dtree_yoff2", "scenery_xoff2", "scenery_yoff2")] + \
               [("tree_depth_scale", C.c_float), ("pad", C.c_uint32)]


class LineTreesIn(C.Structure):  # terra_line_trees_in
    _fields_ = [(k, C.c_void_p) for k in ("zvals", "stats", "is_distant", "pine", "pine_counts", "trunk_override")] + [("pine_capacity", C.c_uint32)] + \
               [(k, C.c_int32) for k in ("dxoff", "dyoff", "ptree_xoff2", "ptree_yoff2")] + [("tree_depth_scale", C.c_float)]


class LineTreeHit(C.Structure):  # terra_line_tree_hit
    _fields_ = [("t", C.c_float), ("tile", C.c_int32), ("xpos", C.c_int32), ("ypos", C.c_int32), ("p_int", C.c_float * 3), ("hit", C.c_uint32), ("tree", C.c_int32),
                ("part", C.c_uint32)]


assert C.sizeof(LineTreesIn) == 72 and C.sizeof(LineTreeHit) == 40


def _address(x):
    """the address of a numpy array, a ctypes object or a DeviceBuffer; an int is taken as an address; None stays None"""
    if x is None or isinstance(x, int):
        return x
    if isinstance(x, np.ndarray):
        assert x.flags["C_CONTIGUOUS"]
        return x.ctypes.data
    return x.ptr if hasattr(x, "ptr") else C.addressof(x)


def make_collide_in(stats=None, trmax=None, tile_zmax=None, flags=None, pine=None, pine_counts=None, trunk_override=None, decid=None, decid_counts=None, scenery=None,
                    scenery_counts=None, radius_override=None, tree_data=None, br_scale=None, pine_capacity=None, decid_capacity=None, scenery_capacity=None,
                    num_tree_data=None, dxoff=0, dyoff=0, ptree_xoff2=0, ptree_yoff2=0, dtree_xoff2=0, dtree_yoff2=0, scenery_xoff2=0, scenery_yoff2=0, tree_depth_scale=1.0):
    """terra_collide_in.  An array is a C-contiguous numpy array, a ctypes object, a DeviceBuffer or an address; host arrays go with the host forms, device memory with
    the _dev forms.  A capacity that is not given is a [n, capacity] numpy array's; num_tree_data the length of tree_data.  The struct keeps its arrays alive."""
    cap = lambda given, arr: int(given) if given is not None else (arr.shape[1] if isinstance(arr, np.ndarray) and arr.ndim == 2 else 0)  # noqa: E731
    ntd = int(num_tree_data) if num_tree_data is not None else (len(tree_data) if isinstance(tree_data, np.ndarray) else 0)
    arrays = (stats, trmax, tile_zmax, flags, pine, pine_counts, trunk_override, decid, decid_counts, scenery, scenery_counts, radius_override, tree_data, br_scale)
    cin = CollideIn(*[_address(x) for x in arrays], cap(pine_capacity, pine), cap(decid_capacity, decid), cap(scenery_capacity, scenery), ntd, dxoff, dyoff, ptree_xoff2,
                    ptree_yoff2, dtree_xoff2, dtree_yoff2, scenery_xoff2, scenery_yoff2, tree_depth_scale, 0)
    cin._keep = arrays
    return cin


def make_line_trees_in(zvals=None, stats=None, is_distant=None, pine=None, pine_counts=None, trunk_override=None, pine_capacity=None, dxoff=0, dyoff=0, ptree_xoff2=0,
                       ptree_yoff2=0, tree_depth_scale=1.0):
    """terra_line_trees_in.  An array is a C-contiguous numpy array, a ctypes object, a DeviceBuffer or an address; host arrays go with the host form, device memory with
    the _dev form.  A capacity that is not given is a [n, capacity] numpy array's.  The struct keeps its arrays alive."""
    cap = int(pine_capacity) if pine_capacity is not None else (pine.shape[1] if isinstance(pine, np.ndarray) and pine.ndim == 2 else 0)
    arrays = (zvals, stats, is_distant, pine, pine_counts, trunk_override)
    lin = LineTreesIn(*[_address(x) for x in arrays], cap, dxoff, dyoff, ptree_xoff2, ptree_yoff2, tree_depth_scale)
    lin._keep = arrays
    return lin


SPHERE_QUERY_DTYPE = np.dtype([("pos", np.float32, (3,)), ("radius", np.float32), ("tile", np.int32), ("flags", np.uint32)])  # terra_sphere_query
SPHERE_HIT_DTYPE = np.dtype([("pos", np.float32, (3,)), ("tile", np.int32), ("word", np.uint32), ("nhits", np.uint32)])      # terra_sphere_hit
assert SPHERE_QUERY_DTYPE.itemsize == 24 and SPHERE_HIT_DTYPE.itemsize == 24 and C.sizeof(CollideIn) == 168
COLL_INC_DTREES, COLL_INC_PTREES, COLL_INC_SCENERY, COLL_INC_ALL = 1, 2, 4, 7  # terra_sphere_query.flags
COLL_TILE_DISTANT, COLL_TILE_NO_SCENERY = 1, 2                                 # the per-tile flag byte of terra_collide_in
COLL_HIT_PINE, COLL_HIT_DECID, COLL_HIT_SCENERY, COLL_ROCK_SHAPE_UNDECIDED, COLL_STAGE_SHIFT, COLL_STAGE_MASK = 1, 2, 4, 8, 8, 0xF00  # terra_sphere_hit.word
COLL_STAGE_TESTED, COLL_STAGE_NO_TILE, COLL_STAGE_DISTANT, COLL_STAGE_OUTSIDE, COLL_STAGE_ABOVE, COLL_STAGE_BAD_QUERY = range(6)
CUBE_INT_HIT, CUBE_INT_NO_TILE, CUBE_INT_BAD_QUERY = 1, 2, 4                   # the result byte of tiles_cube_int_trees


class TreeViewArgs(C.Structure):  # terra_tree_view_args
    _fields_ = [("behind_sphere_mult", C.c_float), ("zoom_f", C.c_float), ("tree_depth_scale", C.c_float), ("window_width", C.c_int32), ("shadow_pass", C.c_int32),
                ("draw_trunks", C.c_int32), ("draw_near_leaves", C.c_int32), ("draw_far_leaves", C.c_int32)]


def make_tree_view_args(behind_sphere_mult=1.0, zoom_f=1.0, tree_depth_scale=1.0, window_width=1920, shadow_pass=0, draw_trunks=1, draw_near_leaves=1, draw_far_leaves=1):
    """terra_tree_view_args: behind_sphere_mult as for the terrain view; the three draw booleans of one draw_pine_tree_bl sweep, in any combination"""
    return TreeViewArgs(behind_sphere_mult, zoom_f, tree_depth_scale, window_width, int(bool(shadow_pass)), int(bool(draw_trunks)), int(bool(draw_near_leaves)),
                        int(bool(draw_far_leaves)))


TREE_VIEW_TILE_DTYPE = np.dtype([("dscale", np.float32), ("weight", np.float32), ("flags", np.uint32), ("num_pine", np.uint32), ("num_palm", np.uint32),
                                 ("num_trees", np.uint32), ("leaf_written", np.uint32), ("pad", np.uint32)])  # terra_tree_view_tile
TREE_VIEW_INST_DTYPE = np.dtype([("id", np.uint32), ("pt", np.float32, (3,))])  # terra_tree_view_inst
TRUNK_OVERRIDE_DTYPE = np.dtype([("p1", np.float32, (3,)), ("p2", np.float32, (3,)), ("r1", np.float32), ("r2", np.float32), ("rotated", np.int32)])  # terra_trunk_override
assert TREE_VIEW_TILE_DTYPE.itemsize == 32 and TREE_VIEW_INST_DTYPE.itemsize == 16 and TRUNK_OVERRIDE_DTYPE.itemsize == 36
TRV_TRUNK_NONE, TRV_TRUNK_POLY_ALL, TRV_TRUNK_POLY_SKIPPED, TRV_TRUNK_POINTS, TRV_TRUNK_MASK = 0, 1, 2, 3, 3  # the flags word of terra_tree_view_tile
TRV_NEAR_LEAVES, TRV_FAR_LEAVES, TRV_DITHERED, TRV_PALMS, TRV_DRAW_ALL_NEAR, TRV_DRAW_ALL_FAR = 0x4, 0x8, 0x10, 0x20, 0x40, 0x80
TRV_ALL_VISIBLE, TRV_NEEDS_HIGH, TRV_NEEDS_LOW, TRV_CONTAINS_CAMERA = 0x100, 0x200, 0x400, 0x800


class SceneryViewArgs(C.Structure):  # terra_scenery_view_args
    _fields_ = [("behind_sphere_mult", C.c_float), ("zoom_f", C.c_float), ("smap_pixel_width", C.c_float), ("window_width", C.c_int32), ("shadow_pass", C.c_int32),
                ("reflection_pass", C.c_int32), ("uw_skip", C.c_int32), ("skip_small_shadow_objs", C.c_int32), ("draw_opaque", C.c_int32), ("draw_leaves", C.c_int32)]


def make_scenery_view_args(behind_sphere_mult=1.0, zoom_f=1.0, smap_pixel_width=0.0, window_width=1920, shadow_pass=0, reflection_pass=0, uw_skip=1, skip_small_shadow_objs=0,
                           draw_opaque=1, draw_leaves=1):
    """terra_scenery_view_args: behind_sphere_mult as for the terrain view; draw_opaque / draw_leaves: the two sweeps of tile_draw_t::draw_scenery, in any combination"""
    return SceneryViewArgs(behind_sphere_mult, zoom_f, smap_pixel_width, window_width, int(bool(shadow_pass)), int(reflection_pass), int(bool(uw_skip)),
                           int(bool(skip_small_shadow_objs)), int(bool(draw_opaque)), int(bool(draw_leaves)))


SCENERY_VIEW_TILE_DTYPE = np.dtype([("dist_scale", np.float32), ("scale_val", np.float32), ("flags", np.uint32), ("num_records", np.uint32), ("list_written", np.uint32),
                                    ("pad", np.uint32, (3,))])  # terra_scenery_view_tile
assert SCENERY_VIEW_TILE_DTYPE.itemsize == 32 and C.sizeof(SceneryViewArgs) == 40
SCV_NONE, SCV_POINT, SCV_LINE, SCV_POLY, SCV_ENGINE, SCV_FORM_MASK = 0, 1, 2, 3, 7, 7  # bits 0-2 of a draw word of tiles_scenery_view
SCV_LOG_END, SCV_LOG_END2, SCV_STUMP_TOP, SCV_CAP_UNDERSIDE, SCV_LEAVES, SCV_UNDERWATER, SCV_BERRIES = 0x8, 0x10, 0x20, 0x40, 0x80, 0x4000, 0x8000
SCV_NDIV_SHIFT, SCV_NDIV_MASK, SCV_BERRY_NDIV_SHIFT = 8, 0x3F, 16
SCV_TILE_DRAWN, SCV_TILE_OPAQUE, SCV_TILE_LEAVES = 1, 2, 4  # the flags word of terra_scenery_view_tile
SCV_GROUPS = ("rock_shape", "surface_rock", "rock", "log", "stump", "mushroom", "stem", "berries", "voxel_rock", "plant_leaves", "leafy_leaves", "pld_points",
              "pld_lines")  # TERRA_SCV_G_*


class DecidViewArgs(C.Structure):  # terra_decid_view_args
    _fields_ = [("behind_sphere_mult", C.c_float), ("zoom_f", C.c_float), ("lod_scales", C.c_float * 4), ("shadow_pass", C.c_int32), ("reflection_pass", C.c_int32),
                ("billboards", C.c_int32), ("leaf_color_changed", C.c_int32), ("draw_leaves", C.c_int32), ("draw_branches", C.c_int32)]


def make_decid_view_args(behind_sphere_mult=1.0, zoom_f=1.0, lod_scales=(0.0, 0.0, 0.0, 0.0), shadow_pass=0, reflection_pass=0, billboards=1, leaf_color_changed=0,
                         draw_leaves=1, draw_branches=1):
    """terra_decid_view_args: behind_sphere_mult as for the terrain view; lod_scales = tree_lod_scales (branch start, branch end, leaf start, leaf end); draw_leaves /
    draw_branches: the two sweeps of tile_draw_t::draw_decid_trees, in any combination"""
    return DecidViewArgs(behind_sphere_mult, zoom_f, (C.c_float * 4)(*[float(x) for x in lod_scales]), int(bool(shadow_pass)), int(reflection_pass), int(bool(billboards)),
                         int(bool(leaf_color_changed)), int(bool(draw_leaves)), int(bool(draw_branches)))


DECID_TREE_DATA_DTYPE = np.dtype([("base_radius", np.float32), ("sphere_radius", np.float32), ("sphere_center_zoff", np.float32), ("lr_z_cent", np.float32),
                                  ("leaves_bcube", np.float32, (6,)), ("branches_bcube", np.float32, (6,)), ("num_leaves", np.uint32), ("num_branch_quads", np.uint32),
                                  ("flags", np.uint32), ("pad", np.uint32)])  # terra_decid_tree_data
DECID_VIEW_TILE_DTYPE = np.dtype([("flags", np.uint32), ("num_trees", np.uint32), ("leaf_written", np.uint32), ("branch_written", np.uint32), ("leaf_bb_written", np.uint32),
                                  ("branch_bb_written", np.uint32), ("pad", np.uint32, (2,))])  # terra_decid_view_tile
DECID_VIEW_BB_DTYPE = np.dtype([("tree_id", np.uint32), ("rec", np.uint32), ("pos", np.float32, (3,)), ("opacity", np.float32)])  # terra_decid_view_bb
assert DECID_TREE_DATA_DTYPE.itemsize == 80 and DECID_VIEW_TILE_DTYPE.itemsize == 32 and DECID_VIEW_BB_DTYPE.itemsize == 24 and C.sizeof(DecidViewArgs) == 48
DCV_GENERATED, DCV_HAS_4TH, DCV_LEAF_TEX, DCV_BRANCH_TEX = 1, 2, 4, 8  # the flags of terra_decid_tree_data
DCV_TILE_DRAWN, DCV_TILE_LEAVES, DCV_TILE_BRANCHES, DCV_TILE_SORTED, DCV_TILE_BCUBE_ZERO_AREA = 1, 2, 4, 8, 16  # the flags word of terra_decid_view_tile
DCV_FORM_NONE, DCV_FORM_GEOM, DCV_FORM_BOTH, DCV_FORM_BILLBOARD, DCV_FORM_MASK, DCV_NOT_VISIBLE, DCV_LOW_DETAIL, DCV_STAGE_SHIFT = 0, 1, 2, 3, 3, 4, 8, 4  # a leaf / branch word
DCV_STAGE_NONE, DCV_STAGE_NOT_VISIBLE, DCV_STAGE_NO_LEAVES, DCV_STAGE_BOX, DCV_STAGE_SIZE, DCV_STAGE_SHADOW_DIST, DCV_STAGE_SHADOW_SPHERE = range(7)


TREE_INST_DTYPE = np.dtype([("type", np.int32), ("height", np.float32), ("width", np.float32)])  # terra_tree_inst
assert TREE_INST_DTYPE.itemsize == 12
TREE_AO_NO_PINE_PALM, TREE_AO_NO_DECID, TREE_AO_DISTANT = 1, 2, 4  # the per-tile flag byte of tiles_tree_ao_shadows
TREE_EDIT_PINE_NOT_GENERATED, TREE_EDIT_DECID_NOT_GENERATED = 1, 2  # the per-tile gen_flags byte of tiles_edit_trees


class TreeSizeParams(C.Structure):  # terra_tree_size_params
    _fields_ = [("tree_height_scale", C.c_float), ("sm_tree_scale", C.c_float), ("pine_tree_radius_scale", C.c_float)]


def make_tree_size_params(tree_height_scale=1.0, sm_tree_scale=1.0, pine_tree_radius_scale=1.0):
    """terra_tree_size_params with the reference's defaults."""
    return TreeSizeParams(tree_height_scale, sm_tree_scale, pine_tree_radius_scale)


class GRASS_BRUSH(C.Structure):
    """terra_grass_brush: one stroke of the fire modes "Add Grass" / "Remove Grass" (tile_t::add_or_remove_grass_at's arguments)"""
    _fields_ = [("pos", C.c_float * 3), ("radius", C.c_float), ("add_grass", C.c_int32), ("shape", C.c_int32), ("brush_weight", C.c_float)]


def make_grass_brush(pos, radius, add_grass, shape, brush_weight):
    return GRASS_BRUSH((C.c_float * 3)(*pos), radius, int(bool(add_grass)), shape, brush_weight)


class ErosionReport(C.Structure):  # terra_erosion_report
    _fields_ = [("droplets", C.c_uint32), ("windows", C.c_uint32), ("rounds", C.c_uint32), ("traces", C.c_uint32),
                ("serial_fallbacks", C.c_uint32), ("nan_droplets", C.c_uint32), ("steps", C.c_uint64), ("traced_steps", C.c_uint64),
                ("retraces_same", C.c_uint64), ("checkpoint_resumes", C.c_uint64), ("checkpoint_steps_saved", C.c_uint64),
                ("window_shifts", C.c_uint64), ("critical_steps", C.c_uint64), ("critical_shifts", C.c_uint64),
                ("clk_wave", C.c_uint64), ("clk_init", C.c_uint64), ("clk_shift", C.c_uint64), ("clk_tail", C.c_uint64), ("clk_critical", C.c_uint64),
                ("clk_shift_flush", C.c_uint64), ("clk_shift_prep", C.c_uint64), ("clk_shift_load", C.c_uint64),
                ("crit_clk_flush", C.c_uint64), ("crit_clk_load", C.c_uint64), ("crit_clk_prep", C.c_uint64),
                ("crit_clk_shift", C.c_uint64), ("crit_clk_edge", C.c_uint64), ("crit_steps_own", C.c_uint64),
                ("sparse_droplets", C.c_uint64), ("sparse_retraces", C.c_uint64), ("sparse_probe_only", C.c_uint64)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


HMAP_ISLANDS = [1000.0, 0, 0, 0, 1000.0, 0, 0, 0, 0, 5.0, 0.001, -4.0, 0, 0]  # hmap_params_t defaults + scene_config/config.txt:76


def make_config(mesh_gen_mode=0, mesh_gen_shape=0, mesh_seed=1, mesh_freq_filter=0, hmap=None, glaciate=1, mesh_scale=1.0,
                mesh_height=0.7, custom_glaciate_exp=0.0, erode_amount=1.0, mesh_xy=128, scene=(4.0, 4.0, 4.0)):
    """The synthetic scene of BASELINE.md section 3 (scene_config/config.txt:56-97)."""
    c = Config()
    c.mesh_x = c.mesh_y = mesh_xy
    c.scene_x, c.scene_y, c.scene_z = scene
    c.mesh_height, c.mesh_scale = mesh_height, mesh_scale
    c.mesh_seed, c.mesh_freq_filter, c.mesh_gen_mode, c.mesh_gen_shape, c.glaciate = mesh_seed, mesh_freq_filter, mesh_gen_mode, mesh_gen_shape, glaciate
    c.custom_glaciate_exp = custom_glaciate_exp
    for i, v in enumerate(HMAP_ISLANDS if hmap is None else hmap):
        c.hmap[i] = v
    c.erode_amount = erode_amount
    c.water_h_off = c.water_h_off_rel = c.relh_adj_tex = c.ocean_wave_height = 0.0
    c.start_mag, c.start_freq, c.mag_mult, c.freq_mult = 0.02, 240.0, 2.0, 0.5
    return c


def default_lib_path():
    """3dworld_amd/libterra_hip.so; TERRA_LIB names another build of the same library (A/B experiments with tools/ab_build.sh -- never set in tests or bench runs)"""
    return os.environ.get("TERRA_LIB") or os.path.join(HERE, "libterra_hip.so")


_vp, _f, _u32, _i32, _sz = C.c_void_p, C.c_float, C.c_uint32, C.c_int, C.c_size_t
_f3 = C.POINTER(C.c_float)

_PROTOS = {
    "terra_last_error": (C.c_char_p, []),
    "terra_device_count": (_i32, []),
    "terra_create": (_i32, [C.POINTER(_vp), _i32]),
    "terra_destroy": (None, [_vp]),
    "terra_set_stream": (_i32, [_vp, _vp]),
    "terra_synchronize": (_i32, [_vp]),
    "terra_set_option": (_i32, [_vp, C.c_char_p, C.c_char_p]),
    "terra_eval_points": (_i32, [_vp, _vp, C.c_uint32, C.c_uint32, C.c_float, _i32, _i32, _i32, _vp]),
    "terra_eval_points_dev": (_i32, [_vp, _vp, C.c_uint32, C.c_uint32, C.c_float, _i32, _i32, _i32, _vp]),
    "terra_host_alloc": (_vp, [_sz]),
    "terra_host_free": (None, [_vp]),
    "terra_download_async": (_i32, [_vp, _vp, _vp, _sz]),
    "terra_download_wait": (_i32, [_vp]),
    "terra_init_scene": (_i32, [_vp, C.POINTER(Config)]),
    "terra_set_config": (_i32, [_vp, C.POINTER(Config)]),
    "terra_get_state": (_i32, [_vp, C.POINTER(State)]),
    "terra_set_state": (_i32, [_vp, C.POINTER(State)]),
    "terra_set_mode": (_i32, [_vp, _i32, _i32]),
    "terra_set_zmax_est": (_i32, [_vp, _f]),
    "terra_set_water_plane_z": (_i32, [_vp, _f]),
    "terra_set_start_eval_sin": (_i32, [_vp, _i32]),
    "terra_set_erode_amount": (_i32, [_vp, _f]),
    "terra_get_max_sea_level": (_f, [_vp]),
    "terra_gen_create": (_i32, [_vp, C.POINTER(_vp)]),
    "terra_gen_destroy": (None, [_vp]),
    "terra_gen_build_arrays": (_i32, [_vp, _f, _f, _f, _f, _u32, _u32, _u32, _i32]),
    "terra_gen_enable_glaciate": (_i32, [_vp]),
    "terra_gen_is_running": (_i32, [_vp]),
    "terra_gen_collect": (_i32, [_vp, _vp]),
    "terra_gen_eval_index": (_f, [_vp, _u32, _u32, _i32, _i32]),
    "terra_gen_grid_rows_minmax_dev": (_i32, [_vp, _f, _f, _f, _f, _u32, _u32, _u32, _i32, _u32, _u32, _vp, _vp, _vp]),
    "terra_gen_device_values": (_vp, [_vp]),
    "terra_gen_grid_dev": (_i32, [_vp, _f, _f, _f, _f, _u32, _u32, _u32, _i32, _vp]),
    "terra_gen_grid": (_i32, [_vp, _f, _f, _f, _f, _u32, _u32, _u32, _i32, _vp]),
    "terra_gen_grid_minmax_dev": (_i32, [_vp, _f, _f, _f, _f, _u32, _u32, _u32, _i32, _vp, _f3, _f3]),
    "terra_eval_mesh_sin_terms": (_i32, [_vp, _f, _f, _f3]),
    "terra_glaciate_mesh_dev": (_i32, [_vp, _vp, _u32, _u32, _i32, _i32, _vp]),
    "terra_apply_erosion_dev": (_i32, [_vp, _vp, _i32, _i32, _f, _u32, _u32]),
    "terra_apply_erosion": (_i32, [_vp, _vp, _i32, _i32, _f, _u32]),
    "terra_release_scratch": (_i32, [_vp]),
    "terra_event_create": (_i32, [_vp, C.POINTER(_vp)]),
    "terra_event_record": (_i32, [_vp, _vp]),
    "terra_event_wait": (_i32, [_vp, _vp]),
    "terra_event_synchronize": (_i32, [_vp]),
    "terra_event_destroy": (None, [_vp]),
    "terra_apply_erosion_devmin_dev": (_i32, [_vp, _vp, _i32, _i32, _vp, _u32, _u32]),
    "terra_erosion_shard_arena_bytes": (C.c_size_t, [_vp, _u32]),
    "terra_erosion_shard_trace_dev": (_i32, [_vp, _vp, _i32, _i32, _u32, _u32, _u32, _vp]),
    "terra_erosion_shard_finish_dev": (_i32, [_vp, _vp, _i32, _i32, _vp, _u32, _u32, _u32, _u32, C.POINTER(_u32), _vp, C.c_size_t]),
    "terra_gen_grid_minmax_async_dev": (_i32, [_vp, _f, _f, _f, _f, _u32, _u32, _u32, _i32, _vp, _vp]),
    "terra_gen_grid_minmax_turn_dev": (_i32, [_vp, _f, _f, _f, _f, _u32, _u32, _u32, _i32, _vp, _vp, _vp, _vp]),
    "terra_gen_grid_rows_minmax_async_dev": (_i32, [_vp, _f, _f, _f, _f, _u32, _u32, _u32, _i32, _u32, _u32, _vp, _vp]),
    "terra_get_erosion_report": (_i32, [_vp, C.POINTER(ErosionReport)]),
    "terra_set_erosion_tuning": (_i32, [_vp, _u32, _u32, _u32]),
    "terra_set_erosion_slice_steps": (_i32, [_vp, _u32]),
    "terra_set_tiled_mesh_ao": (_i32, [_vp, _i32]),
    "terra_heightmap_write_png": (_i32, [C.c_char_p, _vp, _u32, _u32, _i32]),
    "terra_heightmap_read_png": (_i32, [C.c_char_p, _i32, C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_i32), _vp, C.c_size_t]),
    "terra_read_mesh": (_i32, [_vp, C.c_char_p, _f, _vp, _u32, _u32, _vp]),
    "terra_write_mesh": (_i32, [C.c_char_p, _vp, _u32, _u32]),
    "terra_tiles_mesh_shadows_dev": (_i32, [_vp, _vp, _u32, _vp, _f3, _vp]),
    "terra_tiles_mesh_shadows": (_i32, [_vp, _vp, _u32, _vp, _f3, _vp]),
    "terra_tiles_mesh_shadows_halo_dev": (_i32, [_vp, _vp, _u32, _vp, _f3, _vp, _vp, _vp, _vp]),
    "terra_hmap_set_dev": (_i32, [_vp, _vp, _i32, _i32, _i32]),
    "terra_set_mesh_height_scales_for_zval_range": (_i32, [_vp, _f, _f]),
    "terra_set_mesh_file_scale": (_i32, [_vp, _f, _f]),
    "terra_get_mesh_file_scale": (_i32, [_vp, _f3, _f3]),
    "terra_heightmap_to_floats_dev": (_i32, [_vp, _vp, _u32, _u32, _i32, _vp]),
    "terra_heightmap_from_floats_dev": (_i32, [_vp, _vp, _u32, _u32, _i32, _vp, C.POINTER(_u32)]),
    "terra_heightmap_postprocess_dev": (_i32, [_vp, _vp, _u32, _u32, _i32, _u32, _vp, C.POINTER(_u32)]),
    "terra_hmap_apply_brushes_dev": (_i32, [_vp, _vp, _u32, _i32, _u32]),
    "terra_hmap_apply_mods_dev": (_i32, [_vp, _vp, _u32]),
    "terra_hmap_read_and_apply_mod_dev": (_i32, [_vp, C.c_char_p]),
    "terra_hmap_write_mod": (_i32, [C.c_char_p, _vp, _u32, _vp, _u32]),
    "terra_hmap_read_mod": (_i32, [C.c_char_p, _vp, _u32, _vp, _vp, _u32, _vp]),
    "terra_export_heightmap_dev": (_i32, [_vp, _f, _f, _u32, _u32, _vp, _vp, _vp]),
    "terra_write_map_mode_heightmap_image": (_i32, [_vp, C.c_char_p, _f, _f, _u32, _u32]),
    "terra_set_landscape": (_i32, [_vp, _vp]),
    "terra_get_landscape": (_i32, [_vp, _vp]),
    "terra_tiles_terrain_params": (_i32, [_vp, _vp, _u32, _vp]),
    "terra_tiles_create_weights_dev": (_i32, [_vp, _vp, _u32, _vp, _vp, _vp, _vp]),
    "terra_tiles_create_weights": (_i32, [_vp, _vp, _u32, _vp, _vp, _vp, _vp]),
    "terra_tiles_edit_grass_dev": (_i32, [_vp, _vp, _u32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "terra_tiles_edit_grass": (_i32, [_vp, _vp, _u32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "terra_tiles_line_intersect_dev": (_i32, [_vp, _vp, _u32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _u32, _vp]),
    "terra_tiles_line_intersect": (_i32, [_vp, _vp, _u32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _u32, _vp]),
    "terra_tiles_line_intersect_trees_dev": (_i32, [_vp, _vp, _u32, _vp, _vp, _vp, _u32, _vp]),
    "terra_tiles_line_intersect_trees": (_i32, [_vp, _vp, _u32, _vp, _vp, _vp, _u32, _vp]),
    "terra_tiles_tree_map_dev": (_i32, [_vp, _vp, _u32, _i32, _i32, _vp, _vp, _vp, _i32, _vp, _vp]),
    "terra_tiles_tree_map": (_i32, [_vp, _vp, _u32, _i32, _i32, _vp, _vp, _vp, _i32, _vp, _vp]),
    "terra_tiles_shadow_texture_dev": (_i32, [_vp, _u32, _vp, _vp, _vp, _vp, _f, _i32, _vp]),
    "terra_tiles_shadow_texture": (_i32, [_vp, _u32, _vp, _vp, _vp, _vp, _f, _i32, _vp]),
    "terra_tiles_tree_weights_dev": (_i32, [_vp, _u32, _vp, _vp, _vp]),
    "terra_tiles_tree_weights": (_i32, [_vp, _u32, _vp, _vp, _vp]),
    "terra_set_tree_params": (_i32, [_vp, _vp]),
    "terra_get_tree_params": (_i32, [_vp, _vp]),
    "terra_set_height_histogram": (_i32, [_vp, _vp, _u32]),
    "terra_get_height_histogram": (_i32, [_vp, _vp, _u32, _vp]),
    "terra_tiles_place_trees_dev": (_i32, [_vp, _vp, _u32, _i32, _i32, _vp, _vp, _u32, _vp, _vp]),
    "terra_tiles_place_trees": (_i32, [_vp, _vp, _u32, _i32, _i32, _vp, _vp, _u32, _vp, _vp]),
    "terra_tiles_place_trees_brush_dev": (_i32, [_vp, _vp, _u32, _i32, _i32, _vp, _vp, _f3, _f, _i32, _u32, _vp, _vp]),
    "terra_tiles_place_trees_brush": (_i32, [_vp, _vp, _u32, _i32, _i32, _vp, _vp, _f3, _f, _i32, _u32, _vp, _vp]),
    "terra_set_decid_params": (_i32, [_vp, _vp]),
    "terra_get_decid_params": (_i32, [_vp, _vp]),
    "terra_tiles_place_decid_trees_dev": (_i32, [_vp, _vp, _u32, _i32, _i32, _vp, _vp, _vp, _u32, _vp, _vp]),
    "terra_tiles_place_decid_trees": (_i32, [_vp, _vp, _u32, _i32, _i32, _vp, _vp, _vp, _u32, _vp, _vp]),
    "terra_tiles_place_decid_trees_brush_dev": (_i32, [_vp, _vp, _u32, _i32, _i32, _vp, _vp, _vp, _f3, _f, _i32, _u32, _vp, _vp]),
    "terra_tiles_place_decid_trees_brush": (_i32, [_vp, _vp, _u32, _i32, _i32, _vp, _vp, _vp, _f3, _f, _i32, _u32, _vp, _vp]),
    "terra_set_tree_size_params": (_i32, [_vp, _vp]),
    "terra_get_tree_size_params": (_i32, [_vp, _vp]),
    "terra_set_tree_instances": (_i32, [_vp, _vp, _u32]),
    "terra_get_tree_instances": (_i32, [_vp, _vp, _u32, _vp]),
    "terra_tiles_tree_ao_shadows_dev": (_i32, [_vp, _vp, _u32, _i32, _i32, _i32, _i32, _vp, _vp, _u32, _vp, _vp, _u32, _vp, _vp, _u32, _vp, _u32, _vp, _vp, _vp, _vp]),
    "terra_tiles_tree_ao_shadows": (_i32, [_vp, _vp, _u32, _i32, _i32, _i32, _i32, _vp, _vp, _u32, _vp, _vp, _u32, _vp, _vp, _u32, _vp, _u32, _vp, _vp, _vp, _vp]),
    "terra_tiles_edit_trees_dev": (_i32, [_vp, _vp, _u32, _i32, _i32, _i32, _i32, _f3, _f, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _vp, _u32, _vp, _vp, _u32, _vp, _vp, _vp, _vp]),
    "terra_tiles_edit_trees": (_i32, [_vp, _vp, _u32, _i32, _i32, _i32, _i32, _f3, _f, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _vp, _u32, _vp, _vp, _u32, _vp, _vp, _vp, _vp]),
    "terra_set_scenery_params": (_i32, [_vp, _vp]),
    "terra_get_scenery_params": (_i32, [_vp, _vp]),
    "terra_tiles_place_scenery_dev": (_i32, [_vp, _vp, _u32, _i32, _i32, _vp, _u32, _vp, _vp, _vp]),
    "terra_tiles_place_scenery": (_i32, [_vp, _vp, _u32, _i32, _i32, _vp, _u32, _vp, _vp, _vp]),
    "terra_set_flower_params": (_i32, [_vp, _vp]),
    "terra_get_flower_params": (_i32, [_vp, _vp]),
    "terra_tiles_place_flowers_dev": (_i32, [_vp, _vp, _u32, _vp, _vp, _u32, _vp, _vp, _vp]),
    "terra_tiles_place_flowers": (_i32, [_vp, _vp, _u32, _vp, _vp, _u32, _vp, _vp, _vp]),
    "terra_tiles_edit_flowers_dev": (_i32, [_vp, _vp, _u32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp]),
    "terra_tiles_edit_flowers": (_i32, [_vp, _vp, _u32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp]),
    "terra_make_view": (_i32, [_vp, _vp, _vp, C.c_float, C.c_float, C.c_float, C.c_float, _vp]),
    "terra_set_grass_view_params": (_i32, [_vp, _vp]),
    "terra_get_grass_view_params": (_i32, [_vp, _vp]),
    "terra_tiles_grass_view_dev": (_i32, [_vp, _vp, _u32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp]),
    "terra_tiles_grass_view": (_i32, [_vp, _vp, _u32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp]),
    "terra_view_behind_sphere_mult": (_i32, [C.c_float, C.c_float, _vp]),
    "terra_tiles_terrain_view_dev": (_i32, [_vp, _vp, _u32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "terra_tiles_terrain_view": (_i32, [_vp, _vp, _u32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "terra_tiles_reflection_view_dev": (_i32, [_vp, _vp, _u32, _i32, _i32] + [_vp] * 17),
    "terra_tiles_reflection_view": (_i32, [_vp, _vp, _u32, _i32, _i32] + [_vp] * 17),
    "terra_tiles_water_view_dev": (_i32, [_vp, _vp, _u32, _i32, _i32] + [_vp] * 10),
    "terra_tiles_water_view": (_i32, [_vp, _vp, _u32, _i32, _i32] + [_vp] * 10),
    "terra_tiles_smap_plan_dev": (_i32, [_vp, _vp, _u32, _i32, _i32] + [_vp] * 14),
    "terra_tiles_smap_plan": (_i32, [_vp, _vp, _u32, _i32, _i32] + [_vp] * 14),
    "terra_tiles_smap_casters_dev": (_i32, [_vp, _vp, _u32, _i32, _i32, _u32] + [_vp] * 15),
    "terra_tiles_smap_casters": (_i32, [_vp, _vp, _u32, _i32, _i32, _u32] + [_vp] * 15),
    "terra_make_light_view": (_i32, [_vp, _vp, C.c_float, _vp, _vp]),
    "terra_set_cloud_params": (_i32, [_vp, _vp]),
    "terra_get_cloud_params": (_i32, [_vp, _vp]),
    "terra_tiles_update_clouds_dev": (_i32, [_vp, _vp, _u32, _vp, _vp, _vp, _u32, _vp]),
    "terra_tiles_update_clouds": (_i32, [_vp, _vp, _u32, _vp, _vp, _vp, _u32, _vp]),
    "terra_tiles_cloud_view_dev": (_i32, [_vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp]),
    "terra_tiles_cloud_view": (_i32, [_vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp]),
    "terra_tiles_sphere_collide_dev": (_i32, [_vp, _vp, _u32, _vp, _vp, _u32, _vp]),
    "terra_tiles_sphere_collide": (_i32, [_vp, _vp, _u32, _vp, _vp, _u32, _vp]),
    "terra_tiles_cube_int_trees_dev": (_i32, [_vp, _vp, _u32, _vp, _vp, _vp, _u32, _vp, _vp]),
    "terra_tiles_cube_int_trees": (_i32, [_vp, _vp, _u32, _vp, _vp, _vp, _u32, _vp, _vp]),
    "terra_tiles_tree_view_dev": (_i32, [_vp, _vp, _u32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "terra_tiles_tree_view": (_i32, [_vp, _vp, _u32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "terra_tiles_scenery_view_dev": (_i32, [_vp, _vp, _u32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp]),
    "terra_tiles_scenery_view": (_i32, [_vp, _vp, _u32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp]),
    "terra_tiles_decid_view_dev": (_i32, [_vp, _vp, _u32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _u32] + [_vp] * 16),
    "terra_tiles_decid_view": (_i32, [_vp, _vp, _u32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _u32] + [_vp] * 16),
    "terra_tiles_ao_lighting_dev": (_i32, [_vp, _vp, _u32, _vp, _vp]),
    "terra_tiles_ao_lighting": (_i32, [_vp, _vp, _u32, _vp, _vp]),
    "terra_heightmap_proc_gen": (_i32, [_vp, _u32, _u32, _u32, _vp, _f3]),
    "terra_heightmap_proc_gen_dev": (_i32, [_vp, _u32, _u32, _u32, _vp, _vp, _vp]),
    "terra_minmax_dev": (_i32, [_vp, _vp, _sz, _f3, _f3]),
    "terra_quantize16_dev": (_i32, [_vp, _vp, _sz, _f, _f, _vp]),
    "terra_tiles_create_zvals_dev": (_i32, [_vp, _vp, _u32, _u32, _vp, _vp, _vp, _vp]),
    "terra_tiles_post_dev": (_i32, [_vp, _vp, _u32, _vp, _vp, _vp, _vp]),
    "terra_tiles_post": (_i32, [_vp, _vp, _u32, _vp, _vp, _vp, _vp]),
    "terra_tiles_create_zvals": (_i32, [_vp, _vp, _u32, _u32, _vp, _vp, _vp, _vp]),
    "terra_tile_size": (_i32, [_vp, C.POINTER(_u32)]),
    "terra_selftest_hot_sqrt": (C.c_int, [_vp, C.c_uint32, C.POINTER(C.c_uint64)]),
    "terra_voxel_fill_dev": (_i32, [_vp, _vp, _u32, _u32, _u32, _f3, _f3, _f3, _f, _f, _i32, _i32, _i32, _f, _i32]),
    "terra_voxel_fill_slab_dev": (_i32, [_vp, _vp, _u32, _u32, _u32, _f3, _f3, _f3, _f, _f, _i32, _i32, _i32, _f, _i32, _u32, _u32]),
    "terra_voxel_fill": (_i32, [_vp, _vp, _u32, _u32, _u32, _f3, _f3, _f3, _f, _f, _i32, _i32, _i32, _f, _i32]),
    "terra_multi_create": (_i32, [C.POINTER(_vp), C.POINTER(_i32), _u32]),
    "terra_multi_destroy": (None, [_vp]),
    "terra_multi_size": (_u32, [_vp]),
    "terra_multi_ctx": (_vp, [_vp, _u32]),
    "terra_multi_partition": (None, [_u32, _u32, _u32, C.POINTER(_u32), C.POINTER(_u32)]),
    "terra_multi_foreach": (_i32, [_vp, _vp, _vp]),
    "terra_multi_synchronize": (_i32, [_vp]),
    "terra_multi_init_scene": (_i32, [_vp, C.POINTER(Config)]),
    "terra_multi_tiles_create_zvals_dev": (_i32, [_vp, _vp, _u32, _u32, _vp, _vp, _vp, _vp]),
    "terra_multi_tiles_create_zvals": (_i32, [_vp, _vp, _u32, _u32, _vp, _vp, _vp, _vp]),
    "terra_multi_gen_grid_rows_dev": (_i32, [_vp, _f, _f, _f, _f, _u32, _u32, _u32, _i32, _vp, _f3, _f3]),
    "terra_multi_voxel_fill_dev": (_i32, [_vp, _vp, _u32, _u32, _u32, _f3, _f3, _f3, _f, _f, _i32, _i32, _i32, _f, _i32]),
    "terra_multi_tiles_mesh_shadows": (_i32, [_vp, _vp, _u32, _vp, _f3, _vp]),
    "terra_multi_shadow_layout": (_i32, [_vp, _vp, _u32, _f3, _vp, _vp, _vp]),
    "terra_multi_tiles_mesh_shadows_dev": (_i32, [_vp, _vp, _u32, _vp, _f3, _vp]),
    "terra_dgrid_granularity": (_sz, [_vp]),
    "terra_dgrid_create": (_i32, [_vp, _u32, C.POINTER(_sz), _u32, C.POINTER(_vp)]),
    "terra_dgrid_export_fd": (_i32, [_vp, C.POINTER(_i32)]),
    "terra_dgrid_import_fd": (_i32, [_vp, _u32, _i32]),
    "terra_dgrid_map": (_i32, [_vp, C.POINTER(_vp)]),
    "terra_dgrid_destroy": (None, [_vp]),
    "terra_multi_dgrid_create": (_i32, [_vp, C.POINTER(_sz), C.POINTER(_vp), C.POINTER(_vp)]),
    "terra_tiles_mesh_shadows_edges_dev": (_i32, [_vp, _vp, _u32, _vp, _f3, _vp, _vp, _vp, _vp]),
    "terra_malloc": (_i32, [_vp, C.POINTER(_vp), _sz]),
    "terra_free": (_i32, [_vp, _vp]),
    "terra_memcpy_h2d": (_i32, [_vp, _vp, _vp, _sz]),
    "terra_memcpy_d2h": (_i32, [_vp, _vp, _vp, _sz]),
    "terra_timer_start": (_i32, [_vp]),
    "terra_timer_stop": (_i32, [_vp, _f3]),
}
EXPORTED_SYMBOLS = sorted(_PROTOS)


def load_library(path=None):
    path = path or default_lib_path()
    if not os.path.exists(path):
        raise TerraError(-4, f"{path} not found: build it with __graft_entry__.build() (hipcc, gfx950). There is no CPU fall-back.")
    if os.path.abspath(path) == os.path.join(HERE, "libterra_hip.so"):  # the shipped library must be the tree's sources (a .so left by an experiment computes something else)
        from . import build as _build
        if _build.needs_build():
            raise TerraError(-4, f"{path} was not built from the sources in 3dworld_amd/csrc: run __graft_entry__.build()")
    lib = C.CDLL(path)
    for name, (res, args) in _PROTOS.items():
        fn = getattr(lib, name)  # raises AttributeError if the ABI is incomplete
        fn.restype, fn.argtypes = res, args
    return lib


def read_png(path, allow_two_byte_grayscale=True, lib=None):
    """terra_heightmap_read_png without a context (host-only entry point): (h, w) or (h, w, 2) uint8, rows flipped like texture_t::load_png"""
    lib = lib or load_library()
    w, h, nc = _u32(), _u32(), _i32()
    args = (str(path).encode(), int(allow_two_byte_grayscale), C.byref(w), C.byref(h), C.byref(nc))
    if lib.terra_heightmap_read_png(*args, None, 0) < 0:
        raise TerraError(-1, lib.terra_last_error().decode())
    out = np.empty((h.value, w.value, 2) if nc.value == 2 else (h.value, w.value), np.uint8)
    if lib.terra_heightmap_read_png(*args, out.ctypes.data, out.nbytes) < 0:
        raise TerraError(-1, lib.terra_last_error().decode())
    return out


class DeviceBuffer:
    """A device allocation owned through the C ABI (for callers that have no torch tensor to hand over)."""

    def __init__(self, terra, nbytes):
        self.t, self.nbytes = terra, nbytes
        p = _vp()
        terra._ck(terra.lib.terra_malloc(terra.ctx, C.byref(p), nbytes))
        self.ptr = p.value

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        self.t._ck(self.t.lib.terra_memcpy_h2d(self.t.ctx, self.ptr, arr.ctypes.data, arr.nbytes))
        return self

    def download(self, dtype, shape):
        out = np.empty(shape, dtype)
        assert out.nbytes <= self.nbytes
        self.t._ck(self.t.lib.terra_memcpy_d2h(self.t.ctx, out.ctypes.data, self.ptr, out.nbytes))
        return out

    def free(self):
        if self.ptr:
            self.t.lib.terra_free(self.t.ctx, self.ptr)
            self.ptr = None


class PinnedArray:
    """A numpy array over pinned host memory from terra_host_alloc: the DMA target of downloads (no staging copy).  free() it explicitly."""

    def __init__(self, lib, shape, dtype=np.float32):
        self.lib = lib
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        lib.terra_host_alloc.restype = _vp
        self.ptr = lib.terra_host_alloc(max(n, 1))
        if not self.ptr:
            raise TerraError(-1, lib.terra_last_error().decode())
        self.array = np.frombuffer((C.c_uint8 * n).from_address(self.ptr), dtype=dtype).reshape(shape)

    def free(self):
        if self.ptr:
            self.array = None
            self.lib.terra_host_free(self.ptr)
            self.ptr = None


# The library reads no environment variable.  Tests and tools keep their TERRA_* experiment variables: this table turns them into terra_set_option calls
# (variable -> (option key, value when the variable is unset)); Terra.apply_env_options() is called at construction and by whoever changes a variable afterwards.
ENV_OPTIONS = {
    "TERRA_GEN_FUSED": ("gen.fused", "0"), "TERRA_SIMPLE_KERNELS": ("kernels.simple", "0"), "TERRA_GRAPHS": ("graphs", "1"),
    "TERRA_SG_KC": ("sg.kc", "27"), "TERRA_SG_KC_TILES": ("sg.kc_tiles", "27"), "TERRA_SG_ROWGROUP": ("sg.rowgroup", "4"), "TERRA_SG_TURN_ROWS": ("sg.turn_rows", "default"), "TERRA_TILE_EROSION": ("tile_erosion", "lds"),
    "TERRA_WEIGHTS_SIMPLE": ("weights.simple", "0"), "TERRA_VOXELS_COLS": ("voxels.cols", "1"), "TERRA_AO_BANDS": ("ao.bands", "1"), "TERRA_AO_WHOLE": ("ao.whole", "1"), "TERRA_SHADOWS_LEVELS": ("shadows.levels", "0"),
    "TERRA_ERO_SPARSE": ("ero.sparse", "auto"), "TERRA_ERO_SPARSE_RETRACES": ("ero.sparse_retraces", "-1"), "TERRA_ERO_LEAD": ("ero.lead", "2"), "TERRA_ERO_BATCH": ("ero.batch", "0"), "TERRA_ERO_FUSE": ("ero.fuse", "3"),
    "TERRA_ERO_LIVE": ("ero.live", "1"), "TERRA_ERO_DIAG": ("ero.diag", "0"), "TERRA_ERO_CK": ("ero.ck", "default"), "TERRA_ERO_NEAR": ("ero.near", "default"),
    "TERRA_ERO_MEM_BUDGET": ("ero.mem_budget", "-1"),
}


class Terra:
    """One terra_ctx (one GPU, one stream)."""

    def __init__(self, device=0, lib_path=None, env_options=True):
        self.lib = load_library(lib_path)
        ctx = _vp()
        rc = self.lib.terra_create(C.byref(ctx), device)
        if rc != 0:
            raise TerraError(rc, self.lib.terra_last_error().decode())
        self.ctx = ctx
        self._env_applied = {}
        if env_options:
            self.apply_env_options()

    def set_option(self, key, value):
        """terra_set_option: every behaviour switch of the library (include/terra.h lists the keys)"""
        self._ck(self.lib.terra_set_option(self.ctx, str(key).encode(), str(value).encode()))

    def apply_env_options(self):
        """experiment knobs of tests / tools: TERRA_* variables -> options (a variable that is unset puts its option back to the default)"""
        for var, (key, default) in ENV_OPTIONS.items():
            val = os.environ.get(var, default)
            if self._env_applied.get(key, default) != val:
                self.set_option(key, val)
                self._env_applied[key] = val

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.terra_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc < 0:
            raise TerraError(rc, self.lib.terra_last_error().decode())
        return rc

    # ---- scene
    def init_scene(self, cfg):
        self._ck(self.lib.terra_init_scene(self.ctx, C.byref(cfg)))
        return self.state()

    def state(self):
        s = State()
        self._ck(self.lib.terra_get_state(self.ctx, C.byref(s)))
        return s

    def set_state(self, s): self._ck(self.lib.terra_set_state(self.ctx, C.byref(s)))
    def set_config(self, cfg): self._ck(self.lib.terra_set_config(self.ctx, C.byref(cfg)))
    def set_mode(self, mode, shape=0): self._ck(self.lib.terra_set_mode(self.ctx, mode, shape))
    def set_zmax_est(self, v): self._ck(self.lib.terra_set_zmax_est(self.ctx, v))
    def set_water_plane_z(self, v): self._ck(self.lib.terra_set_water_plane_z(self.ctx, v))
    def set_start_eval_sin(self, v): self._ck(self.lib.terra_set_start_eval_sin(self.ctx, v))
    def set_erode_amount(self, v): self._ck(self.lib.terra_set_erode_amount(self.ctx, v))
    def set_stream(self, stream_ptr): self._ck(self.lib.terra_set_stream(self.ctx, stream_ptr))
    def release_scratch(self): self._ck(self.lib.terra_release_scratch(self.ctx))
    def synchronize(self): self._ck(self.lib.terra_synchronize(self.ctx))
    def pinned(self, shape, dtype=np.float32): return PinnedArray(self.lib, shape, dtype)

    def download_async(self, dev_ptr, host_arr):
        """device -> host array (numpy, C-contiguous; pageable or PinnedArray.array) behind everything enqueued so far; returns at once -- complete after download_wait()"""
        assert host_arr.flags["C_CONTIGUOUS"]
        self._ck(self.lib.terra_download_async(self.ctx, dev_ptr, host_arr.ctypes.data, host_arr.nbytes))

    def download_wait(self): self._ck(self.lib.terra_download_wait(self.ctx))
    def max_sea_level(self): return self.lib.terra_get_max_sea_level(self.ctx)
    def alloc(self, nbytes): return DeviceBuffer(self, nbytes)
    def timer_start(self): self._ck(self.lib.terra_timer_start(self.ctx))

    def timer_stop(self):
        ms = C.c_float()
        self._ck(self.lib.terra_timer_stop(self.ctx, C.byref(ms)))
        return ms.value

    # ---- host-buffer drop-ins
    def gen_grid(self, x0, y0, dx, dy, nx, ny, flags=GEN_GLACIATE, min_start_sin=0):
        out = np.empty((ny, nx), np.float32)
        self._ck(self.lib.terra_gen_grid(self.ctx, x0, y0, dx, dy, nx, ny, flags, min_start_sin, out.ctypes.data))
        return out

    def apply_erosion(self, hmap, min_zval, iters):
        assert hmap.dtype == np.float32 and hmap.flags.c_contiguous
        ys, xs = hmap.shape
        self._ck(self.lib.terra_apply_erosion(self.ctx, hmap.ctypes.data, xs, ys, min_zval, iters))
        return hmap

    def set_erosion_tuning(self, window=0, log_capacity_log2=0, block_list_capacity=0):
        self._ck(self.lib.terra_set_erosion_tuning(self.ctx, window, log_capacity_log2, block_list_capacity))

    def set_erosion_slice_steps(self, steps):
        self._ck(self.lib.terra_set_erosion_slice_steps(self.ctx, steps))

    def erosion_report(self):
        r = ErosionReport()
        self._ck(self.lib.terra_get_erosion_report(self.ctx, C.byref(r)))
        return r

    @property
    def tile_size(self):
        """S = the scene's mesh_x (get_tile_size): tiles hold (S+2)^2 zvals, (S+1)^2 normals / AO texels (include/terra.h)"""
        s = _u32()
        self._ck(self.lib.terra_tile_size(self.ctx, C.byref(s)))
        return s.value

    def tiles_create_zvals(self, tile_xy, iters_tt=0, stats=True, normals=True):
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        n = len(txy)
        S = self.tile_size
        z = np.empty((n, S + 2, S + 2), np.float32)
        st = (TileStats * n)() if stats else None
        nm = np.empty((n, S + 1, S + 1, 4), np.uint8) if normals else None
        mnz = np.empty(n, np.float32) if normals else None
        self._ck(self.lib.terra_tiles_create_zvals(self.ctx, txy.ctypes.data, n, iters_tt, z.ctypes.data,
                                                    C.addressof(st) if stats else None, nm.ctypes.data if normals else None,
                                                    mnz.ctypes.data if normals else None))
        return z, st, nm, mnz

    def selftest_hot_sqrt(self, stride=1):
        """disagreements of the droplet step's square roots with sqrtf / the correctly rounded root over every stride-th fp32 bit pattern (must be 0)"""
        n = C.c_uint64(0)
        self._ck(self.lib.terra_selftest_hot_sqrt(self.ctx, stride, C.byref(n)))
        return int(n.value)

    def hmap_set_dev(self, ptr, width=0, height=0, ncolors=2, min_z=None, dz=None):
        """heightmap texture for the tile path (device pointer kept, not copied; None / 0 switches it off)"""
        self._ck(self.lib.terra_hmap_set_dev(self.ctx, ptr, width, height, ncolors))
        if ptr and min_z is not None:
            self._ck(self.lib.terra_set_mesh_height_scales_for_zval_range(self.ctx, min_z, dz))

    def set_mesh_file_scale(self, scale, tz):
        """config `mh_filename <png> <scale> <tz>`: pixel value -> height"""
        self._ck(self.lib.terra_set_mesh_file_scale(self.ctx, scale, tz))

    def get_mesh_file_scale(self):
        a, b = C.c_float(), C.c_float()
        self._ck(self.lib.terra_get_mesh_file_scale(self.ctx, C.byref(a), C.byref(b)))
        return a.value, b.value

    def heightmap_to_floats_dev(self, pix_ptr, width, height, ncolors, vals_ptr):
        self._ck(self.lib.terra_heightmap_to_floats_dev(self.ctx, pix_ptr, width, height, ncolors, vals_ptr))

    def heightmap_from_floats_dev(self, vals_ptr, width, height, ncolors, pix_ptr):
        """-> number of values outside [0, 256) pixel units (the reference asserts on those)"""
        bad = _u32()
        self._ck(self.lib.terra_heightmap_from_floats_dev(self.ctx, vals_ptr, width, height, ncolors, pix_ptr, C.byref(bad)))
        return bad.value

    def heightmap_postprocess_dev(self, pix_ptr, width, height, ncolors, erosion_iters_tt, vals_ptr=None):
        """heightmap_t::postprocess_height in place on the device image -> number of out-of-range values"""
        bad = _u32()
        self._ck(self.lib.terra_heightmap_postprocess_dev(self.ctx, pix_ptr, width, height, ncolors, erosion_iters_tt, vals_ptr, C.byref(bad)))
        return bad.value

    def tiles_mesh_shadows(self, tile_xy, zvals, light_pos):
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        n = len(txy)
        zv = self.tile_size + 2
        z = np.ascontiguousarray(zvals, np.float32).reshape(n, zv, zv)
        sm = np.empty((n, zv, zv), np.uint8)
        lp = (C.c_float * 3)(*light_pos)
        self._ck(self.lib.terra_tiles_mesh_shadows(self.ctx, txy.ctypes.data, n, z.ctypes.data, lp, sm.ctypes.data))
        return sm

    def tiles_mesh_shadows_dev(self, tile_xy, z_ptr, light_pos, smask_ptr):
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        lp = (C.c_float * 3)(*light_pos)
        self._ck(self.lib.terra_tiles_mesh_shadows_dev(self.ctx, txy.ctypes.data, len(txy), z_ptr, lp, smask_ptr))

    def tiles_mesh_shadows_halo_dev(self, tile_xy, z_ptr, light_pos, smask_ptr, edge_in=None, edge_in_present=None, want_edge_out=True):
        """part of a terrain: edge_in (n,2,130) float32 + edge_in_present (n,2) uint8 on the host, returns edge_out (n,2,130) or None"""
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        n = len(txy)
        lp = (C.c_float * 3)(*light_pos)
        ei = np.ascontiguousarray(edge_in, np.float32).reshape(n, 2, 130) if edge_in is not None else None
        ep = np.ascontiguousarray(edge_in_present, np.uint8).reshape(n, 2) if edge_in is not None else None
        eo = np.empty((n, 2, 130), np.float32) if want_edge_out else None
        self._ck(self.lib.terra_tiles_mesh_shadows_halo_dev(self.ctx, txy.ctypes.data, n, z_ptr, lp, smask_ptr,
                                                             ei.ctypes.data if ei is not None else None, ep.ctypes.data if ep is not None else None,
                                                             eo.ctypes.data if eo is not None else None))
        return eo

    def heightmap_write_png(self, path, pixels):
        """pixels: (h, w) uint8 or (h, w, 2) uint8 {lo, hi}"""
        px = np.ascontiguousarray(pixels, np.uint8)
        self._ck(self.lib.terra_heightmap_write_png(str(path).encode(), px.ctypes.data, px.shape[1], px.shape[0], 2 if px.ndim == 3 else 1))

    def heightmap_read_png(self, path, allow_two_byte_grayscale=True):
        w, h, nc = _u32(), _u32(), _i32()
        self._ck(self.lib.terra_heightmap_read_png(str(path).encode(), int(allow_two_byte_grayscale), C.byref(w), C.byref(h), C.byref(nc), None, 0))
        out = np.empty((h.value, w.value, 2) if nc.value == 2 else (h.value, w.value), np.uint8)
        self._ck(self.lib.terra_heightmap_read_png(str(path).encode(), int(allow_two_byte_grayscale), C.byref(w), C.byref(h), C.byref(nc), out.ctypes.data, out.nbytes))
        return out

    def read_mesh(self, path, nx, ny, zmm=0.0):
        """read_mesh (src/mesh_gen.cpp:895-933): -> (mesh [ny, nx] float32 = mesh_file_scale*height + mesh_file_tz, (zbottom, ztop)); the context's zmax_est / zmin / zmax /
        water_plane_z are updated as the reference's globals are"""
        out = np.empty((ny, nx), np.float32)
        zz = np.zeros(2, np.float32)
        self._ck(self.lib.terra_read_mesh(self.ctx, os.fsencode(str(path)), float(zmm), out.ctypes.data, nx, ny, zz.ctypes.data))
        return out, (zz[0], zz[1])

    def write_mesh(self, path, mesh):
        m = np.ascontiguousarray(mesh, np.float32)
        self._ck(self.lib.terra_write_mesh(os.fsencode(str(path)), m.ctypes.data, m.shape[1], m.shape[0]))

    def set_tiled_mesh_ao(self, enable):
        self._ck(self.lib.terra_set_tiled_mesh_ao(self.ctx, int(bool(enable))))

    def hmap_apply_brushes_dev(self, brushes, step_sz=1, num_steps=1):
        b = np.ascontiguousarray(brushes, BRUSH_DTYPE).reshape(-1)
        self._ck(self.lib.terra_hmap_apply_brushes_dev(self.ctx, b.ctypes.data, len(b), step_sz, num_steps))

    def hmap_apply_mods_dev(self, mods):
        m = np.ascontiguousarray(mods, MOD_DTYPE).reshape(-1)
        self._ck(self.lib.terra_hmap_apply_mods_dev(self.ctx, m.ctypes.data, len(m)))

    def hmap_read_and_apply_mod_dev(self, path):
        self._ck(self.lib.terra_hmap_read_and_apply_mod_dev(self.ctx, str(path).encode()))

    def hmap_write_mod(self, path, mods, brushes):
        m = np.ascontiguousarray(mods, MOD_DTYPE).reshape(-1); b = np.ascontiguousarray(brushes, BRUSH_DTYPE).reshape(-1)
        self._ck(self.lib.terra_hmap_write_mod(str(path).encode(), m.ctypes.data, len(m), b.ctypes.data, len(b)))

    def hmap_read_mod(self, path):
        n, nb = _u32(), _u32()
        self._ck(self.lib.terra_hmap_read_mod(str(path).encode(), None, 0, C.byref(n), None, 0, C.byref(nb)))
        m = np.zeros(n.value, MOD_DTYPE); b = np.zeros(nb.value, BRUSH_DTYPE)
        self._ck(self.lib.terra_hmap_read_mod(str(path).encode(), m.ctypes.data, len(m), C.byref(n), b.ctypes.data, len(b), C.byref(nb)))
        return m, b

    def export_heightmap_dev(self, xstart, ystart, width, height, vals_ptr, pix_ptr=None):
        r = (C.c_float * 2)()
        self._ck(self.lib.terra_export_heightmap_dev(self.ctx, xstart, ystart, width, height, vals_ptr, pix_ptr, r))
        return r[0], r[1]

    def write_map_mode_heightmap_image(self, path, xstart, ystart, width, height):
        self._ck(self.lib.terra_write_map_mode_heightmap_image(self.ctx, str(path).encode(), xstart, ystart, width, height))

    def set_landscape(self, ls):
        self._ck(self.lib.terra_set_landscape(self.ctx, C.byref(ls)))

    def get_landscape(self):
        ls = Landscape()
        self._ck(self.lib.terra_get_landscape(self.ctx, C.byref(ls)))
        return ls

    def tiles_terrain_params(self, tile_xy):
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        out = np.empty((len(txy), 2, 2, 3), np.float32)
        self._ck(self.lib.terra_tiles_terrain_params(self.ctx, txy.ctypes.data, len(txy), out.ctypes.data))
        return out

    def tiles_create_weights(self, tile_xy, zvals):
        """-> (weights u8 [n,129,129,4], grass blocks [n,32,32] of GRASS_BLOCK_DTYPE, has_any_grass bool [n])"""
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        n = len(txy)
        z = np.ascontiguousarray(zvals, np.float32).reshape(n, 130, 130)
        w = np.empty((n, 129, 129, 4), np.uint8); gb = np.empty((n, 32, 32), GRASS_BLOCK_DTYPE); hg = np.empty(n, np.uint8)
        self._ck(self.lib.terra_tiles_create_weights(self.ctx, txy.ctypes.data, n, z.ctypes.data, w.ctypes.data, gb.ctypes.data, hg.ctypes.data))
        return w, gb, hg.astype(bool)

    def tiles_edit_grass(self, tile_xy, zvals, stats, brush, weights, blocks, dxoff=0, dyoff=0, is_distant=None):
        """tile_t::add_or_remove_grass_at on every tile of host arrays: weights (u8 [n,129,129,4]) and blocks ([n,32,32] GRASS_BLOCK_DTYPE) are edited in place;
        stats: the TileStats of tiles_create_zvals (a ctypes array); brush: GRASS_BRUSH.  -> (updated bool [n], ranges u32 [n,4] = xl, yl, xh, yh)"""
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        n = len(txy)
        z = np.ascontiguousarray(zvals, np.float32).reshape(n, 130, 130)
        assert weights.flags["C_CONTIGUOUS"] and weights.dtype == np.uint8 and weights.shape == (n, 129, 129, 4)
        assert blocks.flags["C_CONTIGUOUS"] and blocks.dtype == GRASS_BLOCK_DTYPE and blocks.shape == (n, 32, 32)
        st = (TileStats * n).from_buffer_copy(bytes(memoryview(stats).cast("B"))[:n * C.sizeof(TileStats)])
        dist = None if is_distant is None else np.ascontiguousarray(is_distant, np.uint8).reshape(n)
        upd = np.empty(n, np.uint8); rg = np.empty((n, 4), np.uint32)
        self._ck(self.lib.terra_tiles_edit_grass(self.ctx, txy.ctypes.data, n, dxoff, dyoff, z.ctypes.data, C.addressof(st), None if dist is None else dist.ctypes.data,
                                                 C.byref(brush), weights.ctypes.data, blocks.ctypes.data, upd.ctypes.data, rg.ctypes.data))
        return upd.astype(bool), rg

    def tiles_line_intersect(self, tile_xy, zvals, stats, lines, line_tile=None, dxoff=0, dyoff=0, is_distant=None):
        """tile_draw_t::line_intersect_mesh (inc_trees = 0) of every line against host arrays: zvals ([n,S+2,S+2]), stats (the TileStats of tiles_create_zvals),
        lines ([nlines,2,3] = v1, v2); line_tile ([nlines], or None): >= 0 restricts a line to that batch tile.  -> LINE_HIT_DTYPE [nlines]"""
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        n = len(txy)
        S = self.tile_size
        z = np.ascontiguousarray(zvals, np.float32).reshape(n, S + 2, S + 2)
        st = (TileStats * n).from_buffer_copy(bytes(memoryview(stats).cast("B"))[:n * C.sizeof(TileStats)]) if n else None
        ln = np.ascontiguousarray(lines, np.float32).reshape(-1, 2, 3)
        lt = None if line_tile is None else np.ascontiguousarray(line_tile, np.int32).reshape(len(ln))
        dist = None if is_distant is None else np.ascontiguousarray(is_distant, np.uint8).reshape(n)
        hits = np.zeros(len(ln), LINE_HIT_DTYPE)
        self._ck(self.lib.terra_tiles_line_intersect(self.ctx, txy.ctypes.data, n, dxoff, dyoff, z.ctypes.data, C.addressof(st) if n else None,
                                                     None if dist is None else dist.ctypes.data, ln.ctypes.data, None if lt is None else lt.ctypes.data, len(ln), hits.ctypes.data))
        return hits

    def tiles_line_intersect_trees(self, tile_xy, lin, lines, line_tile=None):
        """tile_draw_t::line_intersect_mesh with inc_trees = 1 of every line against host arrays: lin a make_line_trees_in of host arrays, lines ([nlines,2,3] = v1, v2);
        line_tile ([nlines], or None): >= 0 restricts a line to that batch tile.  -> LINE_TREE_HIT_DTYPE [nlines]"""
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        ln = np.ascontiguousarray(lines, np.float32).reshape(-1, 2, 3)
        lt = None if line_tile is None else np.ascontiguousarray(line_tile, np.int32).reshape(len(ln))
        hits = np.zeros(len(ln), LINE_TREE_HIT_DTYPE)
        self._ck(self.lib.terra_tiles_line_intersect_trees(self.ctx, txy.ctypes.data if len(txy) else None, len(txy), C.byref(lin), ln.ctypes.data if len(ln) else None,
                                                           None if lt is None else lt.ctypes.data, len(ln), hits.ctypes.data if len(ln) else None))
        return hits

    @staticmethod
    def _splat_lists(splats, first, n):
        sp = np.ascontiguousarray(splats, TREE_SPLAT_DTYPE).reshape(-1)
        fi = np.ascontiguousarray(first, np.uint32).reshape(-1)
        assert len(fi) == n + 1 and (n == 0 or int(fi[-1]) <= len(sp))
        return sp, fi

    def tiles_tree_map(self, tile_xy, splats, first, reset=True, tree_map=None, dxoff=0, dyoff=0, is_distant=None):
        """tile_t::add_tree_ao_shadow's texel loop for every tile's splat list (TREE_SPLAT_DTYPE; tile t owns splats[first[t]:first[t+1]]), in list order.
        reset: start from an all-255 map; else continue on tree_map (u8 [n,S+1,S+1,2] = {ao, sh}, edited in place).  -> (tree_map, updated bool [n])"""
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        n = len(txy)
        S = self.tile_size
        sp, fi = self._splat_lists(splats, first, n)
        if tree_map is None:
            assert reset
            tree_map = np.empty((n, S + 1, S + 1, 2), np.uint8)
        assert tree_map.flags["C_CONTIGUOUS"] and tree_map.dtype == np.uint8 and tree_map.shape == (n, S + 1, S + 1, 2)
        dist = None if is_distant is None else np.ascontiguousarray(is_distant, np.uint8).reshape(n)
        upd = np.empty(n, np.uint8)
        self._ck(self.lib.terra_tiles_tree_map(self.ctx, txy.ctypes.data, n, dxoff, dyoff, None if dist is None else dist.ctypes.data, sp.ctypes.data if len(sp) else None,
                                               fi.ctypes.data, int(bool(reset)), tree_map.ctypes.data, upd.ctypes.data))
        return tree_map, upd.astype(bool)

    def tiles_shadow_texture(self, n, light_factor, mesh_shadows=True, smask_sun=None, smask_moon=None, ao=None, tree_map=None):
        """tile_t::upload_shadow_map_texture: smask_* u8 [n,S+2,S+2], ao u8 [n,S+1,S+1] (None: 170), tree_map u8 [n,S+1,S+1,2] (None: empty) -> u8 [n,S+1,S+1,4]"""
        S = self.tile_size
        arr = lambda a, shape: None if a is None else np.ascontiguousarray(a, np.uint8).reshape(shape)  # noqa: E731
        sun, moon = arr(smask_sun, (n, S + 2, S + 2)), arr(smask_moon, (n, S + 2, S + 2))
        aov, tm = arr(ao, (n, S + 1, S + 1)), arr(tree_map, (n, S + 1, S + 1, 2))
        out = np.empty((n, S + 1, S + 1, 4), np.uint8)
        ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        self._ck(self.lib.terra_tiles_shadow_texture(self.ctx, n, ptr(sun), ptr(moon), ptr(aov), ptr(tm), light_factor, int(bool(mesh_shadows)), out.ctypes.data))
        return out

    def tiles_tree_weights(self, mesh_weights, tree_map=None):
        """the tree pass of tile_t::create_texture: mesh_weights u8 [n,129,129,4], tree_map u8 [n,129,129,2] (None: plain copy) -> weight_data u8 [n,129,129,4]"""
        w = np.ascontiguousarray(mesh_weights, np.uint8)
        n = len(w)
        tm = None if tree_map is None else np.ascontiguousarray(tree_map, np.uint8).reshape(n, 129, 129, 2)
        out = np.empty((n, 129, 129, 4), np.uint8)
        self._ck(self.lib.terra_tiles_tree_weights(self.ctx, n, w.ctypes.data, None if tm is None else tm.ctypes.data, out.ctypes.data))
        return out

    def set_tree_params(self, tp):
        self._ck(self.lib.terra_set_tree_params(self.ctx, C.byref(tp)))

    def get_tree_params(self):
        tp = TreeParams()
        self._ck(self.lib.terra_get_tree_params(self.ctx, C.byref(tp)))
        return tp

    def set_height_histogram(self, vals):
        """height_histogram (sorted, any length; empty: get_median_height returns its argument)"""
        v = np.ascontiguousarray(vals, np.float32).reshape(-1)
        self._ck(self.lib.terra_set_height_histogram(self.ctx, v.ctypes.data if len(v) else None, len(v)))

    def get_height_histogram(self):
        n = _u32()
        self._ck(self.lib.terra_get_height_histogram(self.ctx, None, 0, C.byref(n)))
        out = np.empty(n.value, np.float32)
        self._ck(self.lib.terra_get_height_histogram(self.ctx, out.ctypes.data if n.value else None, n.value, C.byref(n)))
        return out

    def tiles_place_trees(self, tile_xy, capacity, xoff2=0, yoff2=0, skip=None, stats=None, brush=None):
        """small_tree_group::gen_trees for every tile, or gen_trees_tt_within_radius with brush = (pos[3], radius, is_square).  skip: [n] bytes (can_have_trees()
        false), stats: the TileStats array of tiles_create_zvals.  -> (trees TREE_PLACE_DTYPE [n, capacity], counts uint32 [n]); records past counts[t] are zero"""
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        n = len(txy)
        sk = None if skip is None else np.ascontiguousarray(skip, np.uint8).reshape(n)
        trees, counts = np.zeros((n, capacity), TREE_PLACE_DTYPE), np.zeros(n, np.uint32)
        args = (self.ctx, txy.ctypes.data, n, xoff2, yoff2, None if sk is None else sk.ctypes.data, None if stats is None else C.addressof(stats))
        tail = (capacity, trees.ctypes.data if capacity else None, counts.ctypes.data)
        if brush is None:
            self._ck(self.lib.terra_tiles_place_trees(*args, *tail))
        else:
            pos, radius, is_square = brush
            self._ck(self.lib.terra_tiles_place_trees_brush(*args, (C.c_float * 3)(*pos), radius, int(bool(is_square)), *tail))
        return trees, counts

    def set_decid_params(self, dp):
        self._ck(self.lib.terra_set_decid_params(self.ctx, C.byref(dp)))

    def get_decid_params(self):
        dp = DecidParams()
        self._ck(self.lib.terra_get_decid_params(self.ctx, C.byref(dp)))
        return dp

    def tiles_place_decid_trees(self, tile_xy, capacity, xoff2=0, yoff2=0, skip=None, stats=None, zvals=None, brush=None):
        """tree_cont_t::gen_trees_tt_within_radius for every tile, as gen_deterministic calls it or, with brush = (pos[3], radius, is_square), as add_new_trees does.
        skip: [n] bytes (can_have_trees() false), stats: the TileStats array of tiles_create_zvals, zvals: [n, S+2, S+2] (required with stats).
        -> (trees DECID_PLACE_DTYPE [n, capacity], counts uint32 [n]); records past counts[t] are zero"""
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        n = len(txy)
        sk = None if skip is None else np.ascontiguousarray(skip, np.uint8).reshape(n)
        z = None if zvals is None else np.ascontiguousarray(zvals, np.float32)
        trees, counts = np.zeros((n, capacity), DECID_PLACE_DTYPE), np.zeros(n, np.uint32)
        args = (self.ctx, txy.ctypes.data, n, xoff2, yoff2, None if sk is None else sk.ctypes.data, None if stats is None else C.addressof(stats),
                None if z is None else z.ctypes.data)
        tail = (capacity, trees.ctypes.data if capacity else None, counts.ctypes.data)
        if brush is None:
            self._ck(self.lib.terra_tiles_place_decid_trees(*args, *tail))
        else:
            pos, radius, is_square = brush
            self._ck(self.lib.terra_tiles_place_decid_trees_brush(*args, (C.c_float * 3)(*pos), radius, int(bool(is_square)), *tail))
        return trees, counts

    def set_scenery_params(self, sp):
        self._ck(self.lib.terra_set_scenery_params(self.ctx, C.byref(sp)))

    def get_scenery_params(self):
        sp = SceneryParams()
        self._ck(self.lib.terra_get_scenery_params(self.ctx, C.byref(sp)))
        return sp

    def tiles_place_scenery(self, tile_xy, capacity, xoff2=0, yoff2=0, skip=None, kind_counts=True):
        """the cell loop of scenery_group::gen for every tile, as tile_t::update_scenery calls it.  skip: [n] bytes (update_scenery does not generate).
        -> (objs SCENERY_PLACE_DTYPE [n, capacity], counts uint32 [n], kind_counts uint32 [n, 9] or None); records past counts[t] are zero"""
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        n = len(txy)
        sk = None if skip is None else np.ascontiguousarray(skip, np.uint8).reshape(n)
        objs, counts = np.zeros((n, capacity), SCENERY_PLACE_DTYPE), np.zeros(n, np.uint32)
        kinds = np.zeros((n, len(SCENERY_KINDS)), np.uint32) if kind_counts else None
        self._ck(self.lib.terra_tiles_place_scenery(self.ctx, txy.ctypes.data, n, xoff2, yoff2, None if sk is None else sk.ctypes.data, capacity,
                                                    objs.ctypes.data if capacity else None, counts.ctypes.data, None if kinds is None else kinds.ctypes.data))
        return objs, counts, kinds

    def set_flower_params(self, fp):
        self._ck(self.lib.terra_set_flower_params(self.ctx, C.byref(fp)))

    def get_flower_params(self):
        fp = FlowerParams()
        self._ck(self.lib.terra_get_flower_params(self.ctx, C.byref(fp)))
        return fp

    def tiles_place_flowers(self, tile_xy, weights, capacity, skip=None, aux=True):
        """flower_tile_manager_t::gen_flowers for every tile.  weights: [n, S+1, S+1, 4] bytes as tiles_tree_weights leaves them (None under skip_generate()),
        skip: [n] bytes.  -> (flowers FLOWER_DTYPE [n, capacity], aux uint32 [n, capacity] or None, counts uint32 [n]); records past counts[t] are zero"""
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        n = len(txy)
        sk = None if skip is None else np.ascontiguousarray(skip, np.uint8).reshape(n)
        w = None if weights is None else np.ascontiguousarray(weights, np.uint8)
        flowers, counts = np.zeros((n, capacity), FLOWER_DTYPE), np.zeros(n, np.uint32)
        ax = np.zeros((n, capacity), np.uint32) if aux else None
        self._ck(self.lib.terra_tiles_place_flowers(self.ctx, txy.ctypes.data, n, None if sk is None else sk.ctypes.data, None if w is None else w.ctypes.data, capacity,
                                                    flowers.ctypes.data if capacity else None, None if ax is None else ax.ctypes.data, counts.ctypes.data))
        return flowers, ax, counts

    def tiles_edit_flowers(self, tile_xy, brush, updated, ranges, weights, flowers, aux, counts, generated=None, dxoff=0, dyoff=0):
        """the flowers' half of a grass stroke, in place on flowers [n, capacity] FLOWER_DTYPE, aux [n, capacity] uint32 (or None) and counts [n] uint32; brush,
        updated [n] bytes and ranges [n, 4] uint32 as tiles_edit_grass took and returned them.  -> status uint8 [n]"""
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        n = len(txy)
        assert flowers.dtype == FLOWER_DTYPE and flowers.flags.c_contiguous and counts.dtype == np.uint32 and counts.flags.c_contiguous
        assert aux is None or (aux.dtype == np.uint32 and aux.flags.c_contiguous and aux.shape == flowers.shape)
        capacity = flowers.shape[1]
        up = np.ascontiguousarray(updated, np.uint8).reshape(n)
        rg = None if ranges is None else np.ascontiguousarray(ranges, np.uint32).reshape(n, 4)
        w = None if weights is None else np.ascontiguousarray(weights, np.uint8)
        ge = None if generated is None else np.ascontiguousarray(generated, np.uint8).reshape(n)
        status = np.zeros(n, np.uint8)
        self._ck(self.lib.terra_tiles_edit_flowers(self.ctx, txy.ctypes.data, n, dxoff, dyoff, None if ge is None else ge.ctypes.data, C.byref(brush), up.ctypes.data,
                                                   None if rg is None else rg.ctypes.data, None if w is None else w.ctypes.data, capacity,
                                                   flowers.ctypes.data if capacity else None, None if aux is None else aux.ctypes.data, counts.ctypes.data, status.ctypes.data))
        return status

    def make_view(self, pos, dir, up, angle, aspect, near, far):
        """pos_dir_up's constructor (terra_make_view; no context is involved) -> View"""
        v = View()
        f3 = lambda a: (C.c_float * 3)(*a)  # noqa: E731
        self._ck(self.lib.terra_make_view(f3(pos), f3(dir), f3(up), angle, aspect, near, far, C.byref(v)))
        return v

    def set_grass_view_params(self, gvp):
        self._ck(self.lib.terra_set_grass_view_params(self.ctx, C.byref(gvp)))

    def get_grass_view_params(self):
        gvp = GrassViewParams()
        self._ck(self.lib.terra_get_grass_view_params(self.ctx, C.byref(gvp)))
        return gvp

    def tiles_grass_view(self, tile_xy, zvals, stats, grass_blocks, view, capacity, skip=None, aux=True, want_pass=True, dxoff=0, dyoff=0):
        """tile_t::draw_grass' lists for every tile.  zvals [n, S+2, S+2] float32, stats TileStats * n, grass_blocks [n, dim, dim] GRASS_BLOCK_DTYPE, skip [n] bytes.
        -> (insts float32 [n, capacity, 2], aux uint32 [n, capacity] or None, group_counts uint32 [n, 6, num_rnd_grass_blocks], counts uint32 [n], pass uint8 [n] or
        None); instances past counts[t] are zero.  num_rnd_grass_blocks is read from the context's landscape"""
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        n = len(txy)
        z = np.ascontiguousarray(zvals, np.float32)
        gb = np.ascontiguousarray(grass_blocks, GRASS_BLOCK_DTYPE)
        sk = None if skip is None else np.ascontiguousarray(skip, np.uint8).reshape(n)
        insts, counts = np.zeros((n, capacity, 2), np.float32), np.zeros(n, np.uint32)
        gc = np.zeros((n, GRASS_VIEW_LODS, max(1, int(self.get_landscape().num_rnd_grass_blocks))), np.uint32)
        ax = np.zeros((n, capacity), np.uint32) if aux else None
        ps = np.zeros(n, np.uint8) if want_pass else None
        self._ck(self.lib.terra_tiles_grass_view(self.ctx, txy.ctypes.data, n, dxoff, dyoff, z.ctypes.data, C.addressof(stats) if n else None, gb.ctypes.data,
                                                 None if sk is None else sk.ctypes.data, C.byref(view), capacity, insts.ctypes.data if capacity else None,
                                                 None if ax is None else ax.ctypes.data, gc.ctypes.data, counts.ctypes.data, None if ps is None else ps.ctypes.data))
        return insts, ax, gc, counts, ps

    def view_behind_sphere_mult(self, angle, aspect):
        """pos_dir_up::behind_sphere_mult (terra_view_behind_sphere_mult; no context is involved) -> float"""
        out = C.c_float()
        self._ck(self.lib.terra_view_behind_sphere_mult(angle, aspect, C.byref(out)))
        return out.value

    def tiles_terrain_view(self, tile_xy, stats, view, args, min_normal_z=None, trmax=None, tile_zmax=None, flags=None, occl_state=None, dxoff=0, dyoff=0):
        """the head of tile_draw_t::draw for every tile.  stats TileStats * n; min_normal_z / trmax / tile_zmax [n] float32, flags / occl_state [n] bytes, all optional.
        -> (status uint8 [n], dist float32 [n], lod uint8 [n], crack uint8 [n, 4], draw_order uint32 [counts[0]], occluded uint32 [counts[1]], counts uint32 [2],
        occl_state uint8 [n] after the call or None)"""
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        n = len(txy)
        opt = lambda a, dt: None if a is None else np.array(a, dt).reshape(n)  # noqa: E731  (copies: occl_state is written)
        mn, tr, tz, fl, os_ = opt(min_normal_z, np.float32), opt(trmax, np.float32), opt(tile_zmax, np.float32), opt(flags, np.uint8), opt(occl_state, np.uint8)
        ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        status, dist, lod, crack = np.zeros(n, np.uint8), np.zeros(n, np.float32), np.zeros(n, np.uint8), np.zeros((n, 4), np.uint8)
        order, occluded, counts = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(2, np.uint32)
        self._ck(self.lib.terra_tiles_terrain_view(self.ctx, txy.ctypes.data, n, dxoff, dyoff, C.byref(view), C.byref(args), C.addressof(stats) if n else None, ptr(mn), ptr(tr),
                                                   ptr(tz), ptr(fl), ptr(os_), status.ctypes.data, dist.ctypes.data, lod.ctypes.data, crack.ctypes.data, order.ctypes.data,
                                                   occluded.ctypes.data, counts.ctypes.data, None))
        return status, dist, lod, crack, order[:counts[0]], occluded[:counts[1]], counts, os_

    def tiles_reflection_view(self, tile_xy, stats, view, args, min_normal_z=None, trmax=None, tile_zmax=None, flags=None, occl_state=None, dxoff=0, dyoff=0):
        """tile_draw_t::draw(1) for every tile: tiles_terrain_view's inputs with a ReflectionViewArgs.
        -> (status, dist, lod, crack, draw_order, occluded, counts, occl_state after the call or None, reflect uint8 [n])"""
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        n = len(txy)
        opt = lambda a, dt: None if a is None else np.array(a, dt).reshape(n)  # noqa: E731  (copies: occl_state is written)
        mn, tr, tz, fl, os_ = opt(min_normal_z, np.float32), opt(trmax, np.float32), opt(tile_zmax, np.float32), opt(flags, np.uint8), opt(occl_state, np.uint8)
        ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        status, dist, lod, crack, reflect = np.zeros(n, np.uint8), np.zeros(n, np.float32), np.zeros(n, np.uint8), np.zeros((n, 4), np.uint8), np.zeros(n, np.uint8)
        order, occluded, counts = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(2, np.uint32)
        self._ck(self.lib.terra_tiles_reflection_view(self.ctx, txy.ctypes.data, n, dxoff, dyoff, C.byref(view), C.byref(args), C.addressof(stats) if n else None, ptr(mn), ptr(tr),
                                                      ptr(tz), ptr(fl), ptr(os_), status.ctypes.data, dist.ctypes.data, lod.ctypes.data, crack.ctypes.data, order.ctypes.data,
                                                      occluded.ctypes.data, counts.ctypes.data, None, reflect.ctypes.data))
        return status, dist, lod, crack, order[:counts[0]], occluded[:counts[1]], counts, os_, reflect

    def tiles_water_view(self, tile_xy, stats, view, args, trmax=None, tile_zmax=None, flags=None, status=None, dxoff=0, dyoff=0):
        """is_water_visible() and draw_water_cap's edge tests for every tile: status [n] bytes (optional) is a pass-0 tiles_terrain_view's.
        -> (water_list uint32 [counts[0]], cap_mask uint8 [n] or None, counts uint32 [2]; counts[1] is 0 without status)"""
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        n = len(txy)
        opt = lambda a, dt: None if a is None else np.ascontiguousarray(a, dt).reshape(n)  # noqa: E731
        tr, tz, fl, su = opt(trmax, np.float32), opt(tile_zmax, np.float32), opt(flags, np.uint8), opt(status, np.uint8)
        ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        wl, counts = np.zeros(n, np.uint32), np.zeros(2, np.uint32)
        cm = None if su is None else np.zeros(n, np.uint8)
        self._ck(self.lib.terra_tiles_water_view(self.ctx, txy.ctypes.data, n, dxoff, dyoff, C.byref(view), C.byref(args), C.addressof(stats) if n else None, ptr(tr), ptr(tz), ptr(fl),
                                                 ptr(su), wl.ctypes.data, ptr(cm), counts.ctypes.data))
        return wl[:counts[0]], cm, counts

    def make_light_view(self, lpos, bounds, near_clip=0.01):
        """get_pt_cube_frustum_pdu in its infinite-terrain form (terra_make_light_view; no context is involved): bounds x1 x2 y1 y2 z1 z2 -> (View, behind_sphere_mult)"""
        v, m = View(), C.c_float()
        lp, bd = (C.c_float * 3)(*[float(x) for x in lpos]), (C.c_float * 6)(*[float(x) for x in bounds])
        self._ck(self.lib.terra_make_light_view(lp, bd, near_clip, C.byref(v), C.byref(m)))
        return v, m.value

    def tiles_smap_plan(self, tile_xy, stats, view, args, smap_state, trmax=None, tile_zmax=None, flags=None, terrain_flags=None, want_recomp_order=False, dxoff=0, dyoff=0, fill=None):
        """one frame's shadow-map decisions for every tile.  smap_state [n] bytes (SMAP_NONE or the LOD), terrain_flags [n] bytes or None.  fill: a dict of the outputs'
        initial arrays (the defaults are zeros) -- what the call does not write stays.
        -> dict(plan uint32 [n], dist_scale float32 [n], shadow_bcube float32 [n, 6], receivers uint32 [n], counts uint32 [2], smap_state, terrain_flags, recomp_order or None)"""
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        n = len(txy)
        opt = lambda a, dt: None if a is None else np.array(a, dt).reshape(n)  # noqa: E731  (copies: the state and the flags are written)
        tr, tz, fl, tf, ss = opt(trmax, np.float32), opt(tile_zmax, np.float32), opt(flags, np.uint8), opt(terrain_flags, np.uint8), opt(smap_state, np.uint8)
        ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        fill = fill or {}
        o = dict(plan=np.array(fill.get("plan", np.zeros(n, np.uint32)), np.uint32), dist_scale=np.array(fill.get("dist_scale", np.zeros(n, np.float32)), np.float32),
                 shadow_bcube=np.array(fill.get("shadow_bcube", np.zeros((n, 6), np.float32)), np.float32), receivers=np.array(fill.get("receivers", np.zeros(n, np.uint32)), np.uint32),
                 counts=np.array(fill.get("counts", np.zeros(2, np.uint32)), np.uint32), smap_state=ss, terrain_flags=tf,
                 recomp_order=np.array(fill.get("recomp_order", np.zeros(n, np.uint32)), np.uint32) if want_recomp_order else None)
        self._ck(self.lib.terra_tiles_smap_plan(self.ctx, txy.ctypes.data, n, dxoff, dyoff, C.byref(view), C.byref(args), C.addressof(stats) if n else None, ptr(tr), ptr(tz), ptr(fl),
                                                ptr(ss), o["plan"].ctypes.data, o["dist_scale"].ctypes.data, o["shadow_bcube"].ctypes.data, o["receivers"].ctypes.data,
                                                o["counts"].ctypes.data, ptr(tf), ptr(o["recomp_order"])))
        return o

    @staticmethod
    def _smap_render_arrays(views, bsm, lpos):
        R = len(views)
        va = (View * max(R, 1))(*views)
        return R, va, np.ascontiguousarray(bsm, np.float32).reshape(R), np.ascontiguousarray(lpos, np.float32).reshape(R, 3)

    def tiles_smap_casters(self, tile_xy, stats, recv, views, bsm, lpos, args, trmax=None, tile_zmax=None, flags=None, decid_counts=None, dxoff=0, dyoff=0, fill=None):
        """what is drawn into each receiver's shadow map: recv [R] batch indices, views a list of R View, bsm [R], lpos [R, 3].
        -> dict(to_draw uint32 [R, n], terrain uint32 [R, n], counts uint32 [R, 2], not_drawn uint8 [R, n], status uint8 [R])"""
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        n = len(txy)
        R, va, bm, lp = self._smap_render_arrays(views, bsm, lpos)
        rv = np.ascontiguousarray(recv, np.uint32).reshape(R)
        opt = lambda a, dt: None if a is None else np.ascontiguousarray(a, dt).reshape(n)  # noqa: E731
        tr, tz, fl, dc = opt(trmax, np.float32), opt(tile_zmax, np.float32), opt(flags, np.uint8), opt(decid_counts, np.uint32)
        ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        fill = fill or {}
        o = dict(to_draw=np.array(fill.get("to_draw", np.zeros((R, n), np.uint32)), np.uint32), terrain=np.array(fill.get("terrain", np.zeros((R, n), np.uint32)), np.uint32),
                 counts=np.array(fill.get("counts", np.zeros((R, 2), np.uint32)), np.uint32), not_drawn=np.array(fill.get("not_drawn", np.zeros((R, n), np.uint8)), np.uint8),
                 status=np.array(fill.get("status", np.zeros(R, np.uint8)), np.uint8))
        self._ck(self.lib.terra_tiles_smap_casters(self.ctx, txy.ctypes.data, n, dxoff, dyoff, R, rv.ctypes.data, C.addressof(va), bm.ctypes.data, lp.ctypes.data, C.byref(args),
                                                   C.addressof(stats) if n else None, ptr(tr), ptr(tz), ptr(fl), ptr(dc), o["to_draw"].ctypes.data, o["terrain"].ctypes.data,
                                                   o["counts"].ctypes.data, o["not_drawn"].ctypes.data, o["status"].ctypes.data))
        return o

    def set_cloud_params(self, cp):
        self._ck(self.lib.terra_set_cloud_params(self.ctx, C.byref(cp)))

    def get_cloud_params(self):
        cp = CloudParams()
        self._ck(self.lib.terra_get_cloud_params(self.ctx, C.byref(cp)))
        return cp

    def tiles_update_clouds(self, tile_xy, step, state, clouds):
        """tile_t::update_tile_clouds for every tile in batch order: state CLOUD_TILE_DTYPE [n] and clouds CLOUD_DTYPE [n, capacity], both updated in place (zeroed
        state: a tile that has just entered the batch).  -> total, the sum of the tiles' counts at their turns (the reference's num)"""
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        n = len(txy)
        assert state.dtype == CLOUD_TILE_DTYPE and state.shape == (n,) and state.flags["C_CONTIGUOUS"]
        assert clouds.dtype == CLOUD_DTYPE and clouds.ndim == 2 and clouds.shape[0] == n and clouds.flags["C_CONTIGUOUS"]
        total = np.zeros(1, np.uint32)
        self._ck(self.lib.terra_tiles_update_clouds(self.ctx, txy.ctypes.data, n, C.byref(step), state.ctypes.data if n else None, clouds.ctypes.data if clouds.size else None,
                                                    clouds.shape[1], total.ctypes.data))
        return int(total[0])

    def tiles_cloud_view(self, tile_xy, stats, view, args, state, clouds):
        """get_draw_list for every tile, the sort and tile_cloud_t::draw's decision.  -> (stage uint8 [n, capacity], list CLOUD_INST_DTYPE [list_count], back to front)"""
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        n = len(txy)
        assert state.dtype == CLOUD_TILE_DTYPE and state.shape == (n,) and clouds.dtype == CLOUD_DTYPE and clouds.ndim == 2 and clouds.shape[0] == n
        state, clouds = np.ascontiguousarray(state), np.ascontiguousarray(clouds)
        cap = clouds.shape[1]
        stage, lst, cnt = np.zeros((n, cap), np.uint8), np.zeros(n * cap, CLOUD_INST_DTYPE), np.zeros(1, np.uint32)
        self._ck(self.lib.terra_tiles_cloud_view(self.ctx, txy.ctypes.data, n, C.byref(view), C.byref(args), C.addressof(stats) if n else None, state.ctypes.data if n else None,
                                                 clouds.ctypes.data if clouds.size else None, cap, stage.ctypes.data if stage.size else None, lst.ctypes.data if lst.size else None,
                                                 cnt.ctypes.data))
        return stage, lst[:cnt[0]]

    def tiles_sphere_collide(self, tile_xy, cin, queries):
        """nq calls of tile_draw_t::check_sphere_collision (a query's tile = -1) or tile_t::check_sphere_collision (tile = a batch index) against host arrays:
        cin a make_collide_in of host arrays, queries SPHERE_QUERY_DTYPE [nq].  -> SPHERE_HIT_DTYPE [nq]"""
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        q = np.ascontiguousarray(queries, SPHERE_QUERY_DTYPE).reshape(-1)
        hits = np.zeros(len(q), SPHERE_HIT_DTYPE)
        self._ck(self.lib.terra_tiles_sphere_collide(self.ctx, txy.ctypes.data if len(txy) else None, len(txy), C.byref(cin), q.ctypes.data if len(q) else None, len(q),
                                                     hits.ctypes.data if len(q) else None))
        return hits

    def tiles_cube_int_trees(self, tile_xy, cin, cubes, cube_tile=None):
        """nq calls of tile_draw_t::check_cube_int_trees against host arrays: cubes [nq, 6] = x1 x2 y1 y2 z1 z2, cube_tile [nq] or None.
        -> (result uint8 [nq] of CUBE_INT_*, tile int32 [nq])"""
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        cb = np.ascontiguousarray(cubes, np.float32).reshape(-1, 6)
        ct = None if cube_tile is None else np.ascontiguousarray(cube_tile, np.int32).reshape(len(cb))
        res, tile = np.zeros(len(cb), np.uint8), np.zeros(len(cb), np.int32)
        self._ck(self.lib.terra_tiles_cube_int_trees(self.ctx, txy.ctypes.data if len(txy) else None, len(txy), C.byref(cin), cb.ctypes.data if len(cb) else None,
                                                     None if ct is None or not len(cb) else ct.ctypes.data, len(cb), res.ctypes.data if len(cb) else None,
                                                     tile.ctypes.data if len(cb) else None))
        return res, tile

    def tiles_tree_view(self, tile_xy, stats, view, args, pine, pine_counts, skip=None, trmax=None, trunk_override=None, dxoff=0, dyoff=0, xoff2=0, yoff2=0, fill=0):
        """tile_t::draw_pine_trees for every tile: pine TREE_PLACE_DTYPE [n, cap] with pine_counts [n]; stats TileStats * n; skip [n] bytes, trmax [n] float32,
        trunk_override TRUNK_OVERRIDE_DTYPE [n, cap], all optional.  The [n, cap] outputs start filled with the byte `fill`; entries past the counts keep it.
        -> dict(tile TREE_VIEW_TILE_DTYPE [n], all_bcube float32 [n, 6], pine_insts / palm_insts TREE_VIEW_INST_DTYPE [n, cap], inst_counts uint32 [n, 2],
        leaf_list uint32 [n, cap], leaf_counts uint32 [n, 2], trunk uint8 [n, cap])"""
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        n = len(txy)
        pr = np.ascontiguousarray(pine, TREE_PLACE_DTYPE).reshape(n, -1)
        cap = pr.shape[1]
        pc = np.ascontiguousarray(pine_counts, np.uint32).reshape(n)
        sk = None if skip is None else np.ascontiguousarray(skip, np.uint8).reshape(n)
        tr = None if trmax is None else np.ascontiguousarray(trmax, np.float32).reshape(n)
        ov = None if trunk_override is None else np.ascontiguousarray(trunk_override, TRUNK_OVERRIDE_DTYPE).reshape(n, cap)
        ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        out = self._tree_view_outputs(n, cap, fill)
        self._ck(self.lib.terra_tiles_tree_view(self.ctx, txy.ctypes.data, n, dxoff, dyoff, xoff2, yoff2, C.byref(view), C.byref(args), C.addressof(stats) if n else None, ptr(sk),
                                                ptr(tr), pr.ctypes.data, pc.ctypes.data, cap, ptr(ov), *[out[k].ctypes.data for k in self.TREE_VIEW_OUTPUTS]))
        return out

    TREE_VIEW_OUTPUTS = ("tile", "all_bcube", "pine_insts", "palm_insts", "inst_counts", "leaf_list", "leaf_counts", "trunk")

    @staticmethod
    def _tree_view_outputs(n, cap, fill=0):
        mk = lambda shape, dt: np.frombuffer(bytearray([fill]) * (int(np.prod(shape)) * np.dtype(dt).itemsize), dt).reshape(shape)  # noqa: E731
        return dict(tile=mk((n,), TREE_VIEW_TILE_DTYPE), all_bcube=mk((n, 6), np.float32), pine_insts=mk((n, cap), TREE_VIEW_INST_DTYPE), palm_insts=mk((n, cap), TREE_VIEW_INST_DTYPE),
                    inst_counts=mk((n, 2), np.uint32), leaf_list=mk((n, cap), np.uint32), leaf_counts=mk((n, 2), np.uint32), trunk=mk((n, cap), np.uint8))

    def tiles_scenery_view(self, tile_xy, stats, view, args, objs, counts, list_capacity=None, skip=None, radius_override=None, dxoff=0, dyoff=0, xoff2=0, yoff2=0, fill=0):
        """tile_t::draw_scenery for every tile: objs SCENERY_PLACE_DTYPE [n, cap] with counts [n]; stats TileStats * n; skip [n] bytes and radius_override [n, cap]
        float32 optional; list_capacity defaults to 3*cap.  The [n, cap] and [n, list_capacity] outputs start filled with the byte `fill`; entries past the counts keep it.
        -> dict(tile SCENERY_VIEW_TILE_DTYPE [n], draw uint32 [n, cap], size_scale / dist float32 [n, cap], list uint32 [n, list_capacity], group_counts uint32
        [n, len(SCV_GROUPS)])"""
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        n = len(txy)
        ob = np.ascontiguousarray(objs, SCENERY_PLACE_DTYPE).reshape(n, -1)
        cap = ob.shape[1]
        lcap = 3 * cap if list_capacity is None else int(list_capacity)
        pc = np.ascontiguousarray(counts, np.uint32).reshape(n)
        sk = None if skip is None else np.ascontiguousarray(skip, np.uint8).reshape(n)
        ov = None if radius_override is None else np.ascontiguousarray(radius_override, np.float32).reshape(n, cap)
        ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        out = self._scenery_view_outputs(n, cap, lcap, fill)
        o = [out[k].ctypes.data for k in self.SCENERY_VIEW_OUTPUTS]
        self._ck(self.lib.terra_tiles_scenery_view(self.ctx, txy.ctypes.data, n, dxoff, dyoff, xoff2, yoff2, C.byref(view), C.byref(args), C.addressof(stats) if n else None, ptr(sk),
                                                   ob.ctypes.data, pc.ctypes.data, cap, ptr(ov), *o[:5], lcap, o[5]))
        return out

    SCENERY_VIEW_OUTPUTS = ("tile", "draw", "size_scale", "dist", "list", "group_counts")  # (list_capacity stands between the last two in the C signature)

    @staticmethod
    def _scenery_view_outputs(n, cap, list_cap, fill=0):
        mk = lambda shape, dt: np.frombuffer(bytearray([fill]) * (int(np.prod(shape)) * np.dtype(dt).itemsize), dt).reshape(shape)  # noqa: E731
        return dict(tile=mk((n,), SCENERY_VIEW_TILE_DTYPE), draw=mk((n, cap), np.uint32), size_scale=mk((n, cap), np.float32), dist=mk((n, cap), np.float32),
                    list=mk((n, list_cap), np.uint32), group_counts=mk((n, len(SCV_GROUPS)), np.uint32))

    def tiles_decid_view(self, tile_xy, view, args, tree_data, decid, counts, skip=None, not_visible=None, dxoff=0, dyoff=0, xoff2=0, yoff2=0, fill=0, out=None):
        """tile_t::draw_decid_trees for every tile: decid DECID_PLACE_DTYPE [n, cap] with counts [n]; tree_data DECID_TREE_DATA_DTYPE [num_shared_trees]; skip [n] bytes
        optional; not_visible uint8 [n, cap] optional, read and written in place.  The [n, cap] outputs start filled with the byte `fill` (or are the arrays of `out`);
        entries the call does not write keep it.
        -> dict(tile DECID_VIEW_TILE_DTYPE [n], all_bcube float32 [n, 6], leaf_word / leaf_num / branch_word / branch_num uint32 [n, cap], leaf_scale / leaf_opacity /
        branch_scale / branch_opacity float32 [n, cap], leaf_list / branch_list uint32 [n, cap], leaf_bb / branch_bb DECID_VIEW_BB_DTYPE [n, cap], list_counts uint32 [n, 4])"""
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        n = len(txy)
        dr = np.ascontiguousarray(decid, DECID_PLACE_DTYPE).reshape(n, -1)
        cap = dr.shape[1]
        pc = np.ascontiguousarray(counts, np.uint32).reshape(n)
        td = np.ascontiguousarray(tree_data, DECID_TREE_DATA_DTYPE).reshape(-1)
        sk = None if skip is None else np.ascontiguousarray(skip, np.uint8).reshape(n)
        if not_visible is not None:
            assert not_visible.dtype == np.uint8 and not_visible.shape == (n, cap) and not_visible.flags.c_contiguous and not_visible.flags.writeable
        ptr = lambda a: None if a is None or a.size == 0 else a.ctypes.data  # noqa: E731
        out = self._decid_view_outputs(n, cap, fill) if out is None else out
        self._ck(self.lib.terra_tiles_decid_view(self.ctx, txy.ctypes.data, n, dxoff, dyoff, xoff2, yoff2, C.byref(view), C.byref(args), td.ctypes.data, len(td), ptr(sk), ptr(dr),
                                                 pc.ctypes.data, cap, ptr(not_visible), *[ptr(out[k]) for k in self.DECID_VIEW_OUTPUTS]))
        return out

    DECID_VIEW_OUTPUTS = ("tile", "all_bcube", "leaf_word", "leaf_scale", "leaf_opacity", "leaf_num", "branch_word", "branch_scale", "branch_opacity", "branch_num", "leaf_list",
                          "branch_list", "leaf_bb", "branch_bb", "list_counts")

    @staticmethod
    def _decid_view_outputs(n, cap, fill=0):
        mk = lambda shape, dt: np.frombuffer(bytearray([fill]) * (int(np.prod(shape)) * np.dtype(dt).itemsize), dt).reshape(shape)  # noqa: E731
        u, f = np.uint32, np.float32
        return dict(tile=mk((n,), DECID_VIEW_TILE_DTYPE), all_bcube=mk((n, 6), f), leaf_word=mk((n, cap), u), leaf_scale=mk((n, cap), f), leaf_opacity=mk((n, cap), f),
                    leaf_num=mk((n, cap), u), branch_word=mk((n, cap), u), branch_scale=mk((n, cap), f), branch_opacity=mk((n, cap), f), branch_num=mk((n, cap), u),
                    leaf_list=mk((n, cap), u), branch_list=mk((n, cap), u), leaf_bb=mk((n, cap), DECID_VIEW_BB_DTYPE), branch_bb=mk((n, cap), DECID_VIEW_BB_DTYPE),
                    list_counts=mk((n, 4), u))

    def set_tree_size_params(self, tsp):
        self._ck(self.lib.terra_set_tree_size_params(self.ctx, C.byref(tsp)))

    def get_tree_size_params(self):
        tsp = TreeSizeParams()
        self._ck(self.lib.terra_get_tree_size_params(self.ctx, C.byref(tsp)))
        return tsp

    def set_tree_instances(self, insts):
        """tree_instances as the radii read it: TREE_INST_DTYPE records (type, height, width after the constructor), pines first"""
        v = np.ascontiguousarray(insts, TREE_INST_DTYPE).reshape(-1)
        self._ck(self.lib.terra_set_tree_instances(self.ctx, v.ctypes.data if len(v) else None, len(v)))

    def get_tree_instances(self):
        n = _u32()
        self._ck(self.lib.terra_get_tree_instances(self.ctx, None, 0, C.byref(n)))
        out = np.empty(n.value, TREE_INST_DTYPE)
        self._ck(self.lib.terra_get_tree_instances(self.ctx, out.ctypes.data if n.value else None, n.value, C.byref(n)))
        return out

    def tiles_tree_ao_shadows(self, tile_xy, list_capacity, pine=None, pine_counts=None, decid=None, decid_counts=None, decid_radius=None, decid_radius_by_id=None,
                              flags=None, dxoff=0, dyoff=0, xoff2=0, yoff2=0):
        """tile_t::apply_tree_ao_shadows on the tiles of the batch in batch order, from the placement records: pine TREE_PLACE_DTYPE [n, cap] with pine_counts [n],
        decid DECID_PLACE_DTYPE [n, cap] with decid_counts [n] and decid_radius [n, cap] or decid_radius_by_id [num_shared_trees]; flags: [n] bytes (TREE_AO_*).
        -> (tree_map u8 [n,S+1,S+1,2], updated bool [n], trmax float32 [n], list_counts uint32 [n])"""
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        n = len(txy)
        S = self.tile_size
        ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        pr = None if pine is None else np.ascontiguousarray(pine, TREE_PLACE_DTYPE).reshape(n, -1)
        pc = None if pine_counts is None else np.ascontiguousarray(pine_counts, np.uint32).reshape(n)
        dr = None if decid is None else np.ascontiguousarray(decid, DECID_PLACE_DTYPE).reshape(n, -1)
        dc = None if decid_counts is None else np.ascontiguousarray(decid_counts, np.uint32).reshape(n)
        rr = None if decid_radius is None else np.ascontiguousarray(decid_radius, np.float32).reshape(n, -1)
        assert rr is None or (dr is not None and rr.shape == dr.shape)
        ri = None if decid_radius_by_id is None else np.ascontiguousarray(decid_radius_by_id, np.float32).reshape(-1)
        fl = None if flags is None else np.ascontiguousarray(flags, np.uint8).reshape(n)
        tree_map, upd = np.empty((n, S + 1, S + 1, 2), np.uint8), np.empty(n, np.uint8)
        trmax, lc = np.empty(n, np.float32), np.empty(n, np.uint32)
        self._ck(self.lib.terra_tiles_tree_ao_shadows(self.ctx, txy.ctypes.data, n, dxoff, dyoff, xoff2, yoff2, ptr(pr), ptr(pc), 0 if pr is None else pr.shape[1],
                                                      ptr(dr), ptr(dc), 0 if dr is None else dr.shape[1], ptr(rr), ptr(ri), 0 if ri is None else len(ri), ptr(fl),
                                                      list_capacity, tree_map.ctypes.data, upd.ctypes.data, trmax.ctypes.data, lc.ctypes.data))
        return tree_map, upd.astype(bool), trmax, lc

    def tiles_edit_trees(self, tile_xy, stats, pos, radius, add_trees, is_square, trmax, pine=None, pine_counts=None, decid=None, decid_counts=None, decid_radius=None,
                         decid_radius_by_id=None, skip=None, zvals=None, gen_flags=None, dxoff=0, dyoff=0, xoff2=0, yoff2=0):
        """tile_draw_t::add_or_remove_trees_at on host arrays: pine (TREE_PLACE_DTYPE [n, cap]), pine_counts, decid (DECID_PLACE_DTYPE [n, cap]), decid_counts,
        decid_radius [n, cap] and trmax [n] are edited IN PLACE (they must be C-contiguous arrays of their dtype); stats: the TileStats array of tiles_create_zvals.
        -> (status u8 [n], changed bool [n], update_bcube float32 [6] = x1 x2 y1 y2 z1 z2)"""
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        n = len(txy)
        for a, dt in ((pine, TREE_PLACE_DTYPE), (pine_counts, np.uint32), (decid, DECID_PLACE_DTYPE), (decid_counts, np.uint32), (decid_radius, np.float32), (trmax, np.float32)):
            assert a is None or (a.flags["C_CONTIGUOUS"] and a.dtype == dt)
        assert decid_radius is None or (decid is not None and decid_radius.shape == decid.shape)
        ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        sk = None if skip is None else np.ascontiguousarray(skip, np.uint8).reshape(n)
        gf = None if gen_flags is None else np.ascontiguousarray(gen_flags, np.uint8).reshape(n)
        z = None if zvals is None else np.ascontiguousarray(zvals, np.float32)
        ri = None if decid_radius_by_id is None else np.ascontiguousarray(decid_radius_by_id, np.float32).reshape(-1)
        status, changed, box = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(6, np.float32)
        self._ck(self.lib.terra_tiles_edit_trees(self.ctx, txy.ctypes.data, n, dxoff, dyoff, xoff2, yoff2, (C.c_float * 3)(*pos), radius, int(bool(add_trees)), int(bool(is_square)),
                                                 ptr(sk), C.addressof(stats), ptr(z), ptr(gf), ptr(pine), ptr(pine_counts), 0 if pine is None else pine.shape[1],
                                                 ptr(decid), ptr(decid_counts), 0 if decid is None else decid.shape[1], ptr(decid_radius), ptr(ri), 0 if ri is None else len(ri),
                                                 trmax.ctypes.data, status.ctypes.data, changed.ctypes.data, box.ctypes.data))
        return status, changed.astype(bool), box

    def tiles_ao_lighting(self, tile_xy, zvals):
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        n = len(txy)
        S = self.tile_size
        z = np.ascontiguousarray(zvals, np.float32).reshape(n, S + 2, S + 2)
        ao = np.empty((n, S + 1, S + 1), np.uint8)
        self._ck(self.lib.terra_tiles_ao_lighting(self.ctx, txy.ctypes.data, n, z.ctypes.data, ao.ctypes.data))
        return ao

    def voxel_fill(self, nx, ny, nz, lo_pos, vsz, offset, mag, freq, rseed1, rseed2, gen_mode, zscale, normalize):
        out = np.empty((ny, nx, nz), np.float32)
        a = lambda v: (C.c_float * 3)(*v)
        self._ck(self.lib.terra_voxel_fill(self.ctx, out.ctypes.data, nx, ny, nz, a(lo_pos), a(vsz), a(offset), mag, freq, rseed1, rseed2, gen_mode, zscale, normalize))
        return out

    # ---- device-resident entry points (ptr = raw device pointer, e.g. torch_tensor.data_ptr())
    def gen_grid_dev(self, ptr, x0, y0, dx, dy, nx, ny, flags=GEN_GLACIATE, min_start_sin=0):
        self._ck(self.lib.terra_gen_grid_dev(self.ctx, x0, y0, dx, dy, nx, ny, flags, min_start_sin, ptr))

    def gen_grid_minmax_dev(self, ptr, x0, y0, dx, dy, nx, ny, flags=GEN_GLACIATE, min_start_sin=0):
        mn, mx = C.c_float(), C.c_float()
        self._ck(self.lib.terra_gen_grid_minmax_dev(self.ctx, x0, y0, dx, dy, nx, ny, flags, min_start_sin, ptr, C.byref(mn), C.byref(mx)))
        return mn.value, mx.value

    def gen_grid_rows_minmax_dev(self, ptr, x0, y0, dx, dy, nx, ny, row0, nrows, flags=GEN_GLACIATE, min_start_sin=0, want_minmax=True):
        mn, mx = C.c_float(), C.c_float()
        self._ck(self.lib.terra_gen_grid_rows_minmax_dev(self.ctx, x0, y0, dx, dy, nx, ny, flags, min_start_sin, row0, nrows, ptr,
                                                         C.byref(mn) if want_minmax else None, C.byref(mx) if want_minmax else None))
        return (mn.value, mx.value) if want_minmax else None

    def eval_points(self, xy, exact, xy_scale=1.0, no_xyoff=False, xoff2=0, yoff2=0):
        """terra_eval_points: eval_mesh_sin_terms_scaled (exact=False) / get_exact_zval (exact=True) for the points xy[n][2]"""
        xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        out = np.empty(len(xy), np.float32)
        self._ck(self.lib.terra_eval_points(self.ctx, xy.ctypes.data, len(xy), 1 if exact else 0, xy_scale, int(bool(no_xyoff)), xoff2, yoff2, out.ctypes.data))
        return out

    def eval_points_dev(self, xy_ptr, n, out_ptr, exact, xy_scale=1.0, no_xyoff=False, xoff2=0, yoff2=0):
        self._ck(self.lib.terra_eval_points_dev(self.ctx, xy_ptr, n, 1 if exact else 0, xy_scale, int(bool(no_xyoff)), xoff2, yoff2, out_ptr))

    def eval_mesh_sin_terms(self, xv, yv):
        out = C.c_float()
        self._ck(self.lib.terra_eval_mesh_sin_terms(self.ctx, xv, yv, C.byref(out)))
        return out.value

    def glaciate_mesh_dev(self, ptr, nx, ny, xoff2=0, yoff2=0):
        r = (C.c_float * 2)()
        self._ck(self.lib.terra_glaciate_mesh_dev(self.ctx, ptr, nx, ny, xoff2, yoff2, C.addressof(r)))
        return r[0], r[1]

    def gen_grid_minmax_async_dev(self, ptr, x0, y0, dx, dy, nx, ny, minmax_ptr, flags=GEN_GLACIATE, min_start_sin=0):
        """noise (+ glaciate) with {min, max} left in device memory at minmax_ptr (2 floats); nothing is read back, the call only enqueues"""
        self._ck(self.lib.terra_gen_grid_minmax_async_dev(self.ctx, x0, y0, dx, dy, nx, ny, flags, min_start_sin, ptr, minmax_ptr))

    def gen_grid_minmax_turn_dev(self, ptr, x0, y0, dx, dy, nx, ny, minmax_ptr, wait_for=None, turn=None, flags=GEN_GLACIATE, min_start_sin=0):
        """gen_grid_minmax_async_dev with the noise turn in the call: the map's tables are enqueued at once, the host then waits for event wait_for in front of the grid
        launches, `turn` is recorded while the map's last rows (option sg.turn_rows) are still to be evaluated.  When `turn` fires the map is NOT complete: only this
        context's stream order (or synchronize) says that it is"""
        self._ck(self.lib.terra_gen_grid_minmax_turn_dev(self.ctx, x0, y0, dx, dy, nx, ny, flags, min_start_sin, ptr, minmax_ptr, wait_for, turn))

    def gen_grid_rows_minmax_async_dev(self, ptr, x0, y0, dx, dy, nx, ny, row0, nrows, minmax_ptr, flags=GEN_GLACIATE, min_start_sin=0):
        """rows [row0, row0 + nrows) with the strip's {min, max} left in device memory at minmax_ptr; the call only enqueues"""
        self._ck(self.lib.terra_gen_grid_rows_minmax_async_dev(self.ctx, x0, y0, dx, dy, nx, ny, flags, min_start_sin, row0, nrows, ptr, minmax_ptr))

    def apply_erosion_devmin_dev(self, ptr, xsize, ysize, min_ptr, iters, flags=0):
        """apply_erosion with min_zval read from device memory (one float) when the final clamp runs"""
        self._ck(self.lib.terra_apply_erosion_devmin_dev(self.ctx, ptr, xsize, ysize, min_ptr, iters, flags))

    def erosion_shard_arena_bytes(self, iters):
        """bytes of one rank's arena of a sharded erosion (terra_erosion_shard_*)"""
        return int(self.lib.terra_erosion_shard_arena_bytes(self.ctx, iters))

    def erosion_shard_trace_dev(self, ptr, xsize, ysize, iters, row0, nrows, arena_ptr):
        """probe / trace the droplets that start in rows [row0, row0 + nrows) into this rank's arena (nothing is written to the grid)"""
        self._ck(self.lib.terra_erosion_shard_trace_dev(self.ctx, ptr, xsize, ysize, iters, row0, nrows, arena_ptr))

    def erosion_shard_finish_dev(self, ptr, xsize, ysize, min_ptr, iters, flags, world, self_rank, row_end, arena_self_ptr, arena_stride):
        """the eroding rank: gather the ranks' traces, check / commit / re-trace / clamp = apply_erosion_devmin_dev on the same grid"""
        re = (C.c_uint32 * world)(*[int(v) for v in row_end])
        self._ck(self.lib.terra_erosion_shard_finish_dev(self.ctx, ptr, xsize, ysize, min_ptr, iters, flags, world, self_rank, re, arena_self_ptr, arena_stride))

    def event_create(self):
        e = C.c_void_p()
        self._ck(self.lib.terra_event_create(self.ctx, C.byref(e)))
        return e

    def event_record(self, ev): self._ck(self.lib.terra_event_record(self.ctx, ev))
    def event_wait(self, ev): self._ck(self.lib.terra_event_wait(self.ctx, ev))
    def event_synchronize(self, ev): self._ck(self.lib.terra_event_synchronize(ev))
    def event_destroy(self, ev): self.lib.terra_event_destroy(ev)

    def apply_erosion_dev(self, ptr, xsize, ysize, min_zval, iters, flags=0):
        self._ck(self.lib.terra_apply_erosion_dev(self.ctx, ptr, xsize, ysize, min_zval, iters, flags))

    def heightmap_proc_gen_dev(self, ptr, width, height, erosion_iters, pix_ptr=None):
        rng = (C.c_float * 2)()
        self._ck(self.lib.terra_heightmap_proc_gen_dev(self.ctx, width, height, erosion_iters, ptr, pix_ptr, C.addressof(rng)))
        return rng[0], rng[1]

    def heightmap_proc_gen(self, width, height, erosion_iters):
        """-> (pixels u8 [h, w, 2], min_z, dz): heightmap_t::proc_gen's texture on the host"""
        pix = np.empty((height, width, 2), np.uint8)
        rng = (C.c_float * 2)()
        self._ck(self.lib.terra_heightmap_proc_gen(self.ctx, width, height, erosion_iters, pix.ctypes.data, rng))
        return pix, rng[0], rng[1]

    def minmax_dev(self, ptr, n):
        mn, mx = C.c_float(), C.c_float()
        self._ck(self.lib.terra_minmax_dev(self.ctx, ptr, n, C.byref(mn), C.byref(mx)))
        return mn.value, mx.value

    def quantize16_dev(self, ptr, n, min_z, dz, pix_ptr):
        self._ck(self.lib.terra_quantize16_dev(self.ctx, ptr, n, min_z, dz, pix_ptr))

    def tiles_create_zvals_dev(self, tile_xy, iters_tt, z_ptr, stats_ptr=None, normals_ptr=None, mnz_ptr=None):
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        self._ck(self.lib.terra_tiles_create_zvals_dev(self.ctx, txy.ctypes.data, len(txy), iters_tt, z_ptr, stats_ptr, normals_ptr, mnz_ptr))

    def tiles_post_dev(self, tile_xy, z_ptr, stats_ptr=None, normals_ptr=None, mnz_ptr=None):
        """sub-block ranges / water bbox / radius and normals of zvals the caller has (tile_t::create_zvals' last loop + upload_normal_texture)"""
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        self._ck(self.lib.terra_tiles_post_dev(self.ctx, txy.ctypes.data, len(txy), z_ptr, stats_ptr, normals_ptr, mnz_ptr))

    def tiles_create_weights_dev(self, tile_xy, z_ptr, weights_ptr, blocks_ptr=None, has_grass_ptr=None):
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        self._ck(self.lib.terra_tiles_create_weights_dev(self.ctx, txy.ctypes.data, len(txy), z_ptr, weights_ptr, blocks_ptr, has_grass_ptr))

    def tiles_edit_grass_dev(self, tile_xy, z_ptr, stats_ptr, brush, weights_ptr, blocks_ptr, updated_ptr, ranges_ptr=None, dxoff=0, dyoff=0, distant_ptr=None):
        """the grass brush on device-resident weights / grass blocks, in place; updated_ptr: n bytes, ranges_ptr: n x 4 uint32 (or None).  Only enqueues."""
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        self._ck(self.lib.terra_tiles_edit_grass_dev(self.ctx, txy.ctypes.data, len(txy), dxoff, dyoff, z_ptr, stats_ptr, distant_ptr, C.byref(brush),
                                                     weights_ptr, blocks_ptr, updated_ptr, ranges_ptr))

    def tiles_line_intersect_dev(self, tile_xy, z_ptr, stats_ptr, lines_ptr, nlines, hits_ptr, line_tile_ptr=None, dxoff=0, dyoff=0, distant_ptr=None):
        """line hits against a device-resident batch: lines_ptr [nlines][2][3] floats, hits_ptr nlines x LINE_HIT_DTYPE, line_tile_ptr [nlines] int32 (or None).  Only enqueues."""
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        self._ck(self.lib.terra_tiles_line_intersect_dev(self.ctx, txy.ctypes.data, len(txy), dxoff, dyoff, z_ptr, stats_ptr, distant_ptr, lines_ptr, line_tile_ptr,
                                                         nlines, hits_ptr))

    def tiles_tree_map_dev(self, tile_xy, splats_ptr, first, tree_map_ptr, updated_ptr=None, reset=True, dxoff=0, dyoff=0, distant_ptr=None):
        """the tree map of a device-resident batch: splats_ptr = device TREE_SPLAT_DTYPE records, first = HOST [n+1] uint32, tree_map_ptr [n][S+1][S+1][2] bytes,
        updated_ptr n bytes (or None).  Only enqueues."""
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        fi = np.ascontiguousarray(first, np.uint32).reshape(-1)
        assert len(fi) == len(txy) + 1
        self._ck(self.lib.terra_tiles_tree_map_dev(self.ctx, txy.ctypes.data, len(txy), dxoff, dyoff, distant_ptr, splats_ptr, fi.ctypes.data, int(bool(reset)),
                                                   tree_map_ptr, updated_ptr))

    def tiles_shadow_texture_dev(self, n, light_factor, shadow_ptr, mesh_shadows=True, smask_sun_ptr=None, smask_moon_ptr=None, ao_ptr=None, tree_map_ptr=None):
        """the shadow texture of a device-resident batch: shadow_ptr [n][S+1][S+1][4] bytes.  Only enqueues."""
        self._ck(self.lib.terra_tiles_shadow_texture_dev(self.ctx, n, smask_sun_ptr, smask_moon_ptr, ao_ptr, tree_map_ptr, light_factor, int(bool(mesh_shadows)), shadow_ptr))

    def tiles_tree_weights_dev(self, n, mesh_weights_ptr, tree_map_ptr, weights_ptr):
        """weight_data from mesh_weight_data and the tree map on the device; weights_ptr may be mesh_weights_ptr.  Only enqueues."""
        self._ck(self.lib.terra_tiles_tree_weights_dev(self.ctx, n, mesh_weights_ptr, tree_map_ptr, weights_ptr))

    def tiles_place_trees_dev(self, tile_xy, capacity, trees_ptr, counts_ptr, xoff2=0, yoff2=0, skip_ptr=None, stats_ptr=None, brush=None):
        """tree placement of a device-resident batch: trees_ptr [n][capacity] TREE_PLACE_DTYPE records, counts_ptr [n] uint32, skip_ptr [n] bytes / stats_ptr [n]
        terra_tile_stats (or None).  brush = (pos[3], radius, is_square) for the brush form.  Only enqueues."""
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        args = (self.ctx, txy.ctypes.data, len(txy), xoff2, yoff2, skip_ptr, stats_ptr)
        if brush is None:
            self._ck(self.lib.terra_tiles_place_trees_dev(*args, capacity, trees_ptr, counts_ptr))
        else:
            pos, radius, is_square = brush
            self._ck(self.lib.terra_tiles_place_trees_brush_dev(*args, (C.c_float * 3)(*pos), radius, int(bool(is_square)), capacity, trees_ptr, counts_ptr))

    def tiles_place_decid_trees_dev(self, tile_xy, capacity, trees_ptr, counts_ptr, xoff2=0, yoff2=0, skip_ptr=None, stats_ptr=None, z_ptr=None, brush=None):
        """deciduous tree placement of a device-resident batch: trees_ptr [n][capacity] DECID_PLACE_DTYPE records, counts_ptr [n] uint32, skip_ptr [n] bytes /
        stats_ptr [n] terra_tile_stats / z_ptr [n][S+2][S+2] floats (or None; z_ptr is required with stats_ptr).  brush = (pos[3], radius, is_square) for the brush
        form.  Only enqueues."""
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        args = (self.ctx, txy.ctypes.data, len(txy), xoff2, yoff2, skip_ptr, stats_ptr, z_ptr)
        if brush is None:
            self._ck(self.lib.terra_tiles_place_decid_trees_dev(*args, capacity, trees_ptr, counts_ptr))
        else:
            pos, radius, is_square = brush
            self._ck(self.lib.terra_tiles_place_decid_trees_brush_dev(*args, (C.c_float * 3)(*pos), radius, int(bool(is_square)), capacity, trees_ptr, counts_ptr))

    def tiles_place_scenery_dev(self, tile_xy, capacity, objs_ptr, counts_ptr, xoff2=0, yoff2=0, skip_ptr=None, kind_counts_ptr=None):
        """scenery placement of a device-resident batch: objs_ptr [n][capacity] SCENERY_PLACE_DTYPE records, counts_ptr [n] uint32, skip_ptr [n] bytes or None,
        kind_counts_ptr [n][9] uint32 or None.  Only enqueues."""
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        self._ck(self.lib.terra_tiles_place_scenery_dev(self.ctx, txy.ctypes.data, len(txy), xoff2, yoff2, skip_ptr, capacity, objs_ptr, counts_ptr, kind_counts_ptr))

    def tiles_place_flowers_dev(self, tile_xy, weights_ptr, capacity, flowers_ptr, counts_ptr, aux_ptr=None, skip_ptr=None):
        """the flowers of a device-resident batch: weights_ptr [n][S+1][S+1][4] bytes, flowers_ptr [n][capacity] FLOWER_DTYPE records, aux_ptr [n][capacity] uint32 or
        None, counts_ptr [n] uint32, skip_ptr [n] bytes or None.  Only enqueues."""
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        self._ck(self.lib.terra_tiles_place_flowers_dev(self.ctx, txy.ctypes.data, len(txy), skip_ptr, weights_ptr, capacity, flowers_ptr, aux_ptr, counts_ptr))

    def tiles_edit_flowers_dev(self, tile_xy, brush, updated_ptr, ranges_ptr, weights_ptr, capacity, flowers_ptr, counts_ptr, status_ptr, aux_ptr=None, generated_ptr=None,
                               dxoff=0, dyoff=0):
        """the flowers' half of a grass stroke on device-resident records, in place: updated_ptr / ranges_ptr as tiles_edit_grass_dev left them, status_ptr n bytes.
        Only enqueues."""
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        self._ck(self.lib.terra_tiles_edit_flowers_dev(self.ctx, txy.ctypes.data, len(txy), dxoff, dyoff, generated_ptr, C.byref(brush), updated_ptr, ranges_ptr, weights_ptr,
                                                       capacity, flowers_ptr, aux_ptr, counts_ptr, status_ptr))

    def tiles_grass_view_dev(self, tile_xy, zvals_ptr, stats_ptr, grass_blocks_ptr, view, capacity, insts_ptr, group_counts_ptr, counts_ptr, aux_ptr=None, pass_ptr=None,
                             skip_ptr=None, dxoff=0, dyoff=0):
        """the grass draw lists of a device-resident batch: insts_ptr [n][capacity][2] floats, group_counts_ptr [n][6][num_rnd_grass_blocks] uint32, counts_ptr [n]
        uint32, aux_ptr [n][capacity] uint32 or None, pass_ptr / skip_ptr [n] bytes or None.  view is a host View.  Only enqueues."""
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        self._ck(self.lib.terra_tiles_grass_view_dev(self.ctx, txy.ctypes.data, len(txy), dxoff, dyoff, zvals_ptr, stats_ptr, grass_blocks_ptr, skip_ptr, C.byref(view), capacity,
                                                     insts_ptr, aux_ptr, group_counts_ptr, counts_ptr, pass_ptr))

    def tiles_terrain_view_dev(self, tile_xy, view, args, stats_ptr, status_ptr, dist_ptr, lod_ptr, crack_ptr, draw_order_ptr, occluded_ptr, counts_ptr, min_normal_z_ptr=None,
                               trmax_ptr=None, tile_zmax_ptr=None, flags_ptr=None, occl_state_ptr=None, not_drawn_ptr=None, dxoff=0, dyoff=0):
        """the terrain draw list of a device-resident batch: status_ptr / lod_ptr [n] bytes, dist_ptr [n] floats, crack_ptr [n][4] bytes, draw_order_ptr / occluded_ptr [n]
        uint32, counts_ptr [2] uint32; not_drawn_ptr [n] bytes or None (the grass view's skip bytes); the optional per-tile arrays as in tiles_terrain_view.  view and args are host structs.  Only enqueues."""
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        self._ck(self.lib.terra_tiles_terrain_view_dev(self.ctx, txy.ctypes.data, len(txy), dxoff, dyoff, C.byref(view), C.byref(args), stats_ptr, min_normal_z_ptr, trmax_ptr,
                                                       tile_zmax_ptr, flags_ptr, occl_state_ptr, status_ptr, dist_ptr, lod_ptr, crack_ptr, draw_order_ptr, occluded_ptr, counts_ptr, not_drawn_ptr))

    def tiles_reflection_view_dev(self, tile_xy, view, args, stats_ptr, status_ptr, dist_ptr, lod_ptr, crack_ptr, draw_order_ptr, occluded_ptr, counts_ptr, min_normal_z_ptr=None,
                                  trmax_ptr=None, tile_zmax_ptr=None, flags_ptr=None, occl_state_ptr=None, not_drawn_ptr=None, reflect_ptr=None, dxoff=0, dyoff=0):
        """the terrain draw list of reflection pass 1 of a device-resident batch: tiles_terrain_view_dev's arrays, args a ReflectionViewArgs, reflect_ptr [n] bytes or None.  Only enqueues."""
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        self._ck(self.lib.terra_tiles_reflection_view_dev(self.ctx, txy.ctypes.data, len(txy), dxoff, dyoff, C.byref(view), C.byref(args), stats_ptr, min_normal_z_ptr, trmax_ptr,
                                                          tile_zmax_ptr, flags_ptr, occl_state_ptr, status_ptr, dist_ptr, lod_ptr, crack_ptr, draw_order_ptr, occluded_ptr, counts_ptr,
                                                          not_drawn_ptr, reflect_ptr))

    def tiles_water_view_dev(self, tile_xy, view, args, stats_ptr, water_list_ptr, counts_ptr, status_ptr=None, cap_mask_ptr=None, trmax_ptr=None, tile_zmax_ptr=None, flags_ptr=None,
                             dxoff=0, dyoff=0):
        """water quads and water caps of a device-resident batch: water_list_ptr [n] uint32, counts_ptr [2] uint32; status_ptr (a pass-0 terrain view's) and cap_mask_ptr [n] bytes,
        both or neither.  Only enqueues."""
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        self._ck(self.lib.terra_tiles_water_view_dev(self.ctx, txy.ctypes.data, len(txy), dxoff, dyoff, C.byref(view), C.byref(args), stats_ptr, trmax_ptr, tile_zmax_ptr, flags_ptr,
                                                     status_ptr, water_list_ptr, cap_mask_ptr, counts_ptr))

    def tiles_smap_plan_dev(self, tile_xy, view, args, stats_ptr, smap_state_ptr, plan_ptr, dist_scale_ptr, shadow_bcube_ptr, receivers_ptr, counts_ptr, trmax_ptr=None,
                            tile_zmax_ptr=None, flags_ptr=None, terrain_flags_ptr=None, recomp_order_ptr=None, dxoff=0, dyoff=0):
        """one frame's shadow-map decisions of a device-resident batch: smap_state_ptr [n] bytes (read and written), plan_ptr / receivers_ptr [n] uint32, dist_scale_ptr [n]
        floats, shadow_bcube_ptr [n][6] floats, counts_ptr [2] uint32; terrain_flags_ptr [n] bytes and recomp_order_ptr [n] uint32 or None.  view and args are host structs.
        Only enqueues."""
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        self._ck(self.lib.terra_tiles_smap_plan_dev(self.ctx, txy.ctypes.data, len(txy), dxoff, dyoff, C.byref(view), C.byref(args), stats_ptr, trmax_ptr, tile_zmax_ptr, flags_ptr,
                                                    smap_state_ptr, plan_ptr, dist_scale_ptr, shadow_bcube_ptr, receivers_ptr, counts_ptr, terrain_flags_ptr, recomp_order_ptr))

    def tiles_smap_casters_dev(self, tile_xy, recv_ptr, views, bsm, lpos, args, stats_ptr, to_draw_ptr, terrain_ptr, counts_ptr, not_drawn_ptr, status_ptr, trmax_ptr=None,
                               tile_zmax_ptr=None, flags_ptr=None, decid_counts_ptr=None, dxoff=0, dyoff=0):
        """the casters of R renders on a device-resident batch: recv_ptr [R] uint32 on the device; views (a list of R View), bsm [R] and lpos [R, 3] on the host;
        to_draw_ptr / terrain_ptr [R][n] uint32, counts_ptr [R][2] uint32, not_drawn_ptr [R][n] bytes, status_ptr [R] bytes.  Only enqueues."""
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        R, va, bm, lp = self._smap_render_arrays(views, bsm, lpos)
        self._ck(self.lib.terra_tiles_smap_casters_dev(self.ctx, txy.ctypes.data, len(txy), dxoff, dyoff, R, recv_ptr, C.addressof(va), bm.ctypes.data, lp.ctypes.data, C.byref(args),
                                                       stats_ptr, trmax_ptr, tile_zmax_ptr, flags_ptr, decid_counts_ptr, to_draw_ptr, terrain_ptr, counts_ptr, not_drawn_ptr, status_ptr))

    def tiles_update_clouds_dev(self, tile_xy, step, state_ptr, clouds_ptr, capacity, total_ptr=None):
        """update_tile_clouds of a device-resident batch: state_ptr [n] terra_cloud_tile, clouds_ptr [n][capacity] terra_cloud, total_ptr one uint32 or None.  Only enqueues."""
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        self._ck(self.lib.terra_tiles_update_clouds_dev(self.ctx, txy.ctypes.data, len(txy), C.byref(step), state_ptr, clouds_ptr, capacity, total_ptr))

    def tiles_cloud_view_dev(self, tile_xy, view, args, stats_ptr, state_ptr, clouds_ptr, capacity, stage_ptr, list_ptr, list_count_ptr):
        """the cloud draw list of a device-resident batch: stage_ptr [n][capacity] bytes, list_ptr [n*capacity] terra_cloud_inst, list_count_ptr one uint32.  Only enqueues."""
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        self._ck(self.lib.terra_tiles_cloud_view_dev(self.ctx, txy.ctypes.data, len(txy), C.byref(view), C.byref(args), stats_ptr, state_ptr, clouds_ptr, capacity, stage_ptr, list_ptr,
                                                     list_count_ptr))

    def tiles_line_intersect_trees_dev(self, tile_xy, lin, lines_ptr, nlines, hits_ptr, line_tile_ptr=None):
        """line hits with inc_trees = 1 against a device-resident batch: lin a make_line_trees_in of device arrays, lines_ptr [nlines][2][3] floats, hits_ptr nlines x
        LINE_TREE_HIT_DTYPE, line_tile_ptr [nlines] int32 (or None).  Only enqueues."""
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        self._ck(self.lib.terra_tiles_line_intersect_trees_dev(self.ctx, txy.ctypes.data if len(txy) else None, len(txy), C.byref(lin), lines_ptr, line_tile_ptr, nlines, hits_ptr))

    def tiles_sphere_collide_dev(self, tile_xy, cin, queries_ptr, nq, hits_ptr):
        """the sphere queries of a device-resident batch: cin a make_collide_in of device arrays, queries_ptr [nq] terra_sphere_query, hits_ptr [nq] terra_sphere_hit.
        Only enqueues."""
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        self._ck(self.lib.terra_tiles_sphere_collide_dev(self.ctx, txy.ctypes.data if len(txy) else None, len(txy), C.byref(cin), queries_ptr, nq, hits_ptr))

    def tiles_cube_int_trees_dev(self, tile_xy, cin, cubes_ptr, nq, result_ptr, cube_tile_ptr=None, tile_out_ptr=None):
        """the tree box tests of a device-resident batch: cubes_ptr [nq][6] floats, result_ptr [nq] bytes, cube_tile_ptr / tile_out_ptr [nq] int32 or None.  Only enqueues."""
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        self._ck(self.lib.terra_tiles_cube_int_trees_dev(self.ctx, txy.ctypes.data if len(txy) else None, len(txy), C.byref(cin), cubes_ptr, cube_tile_ptr, nq, result_ptr,
                                                         tile_out_ptr))

    def tiles_tree_view_dev(self, tile_xy, view, args, stats_ptr, pine_ptr, pine_counts_ptr, capacity, tile_out_ptr, all_bcube_ptr, pine_insts_ptr, palm_insts_ptr, inst_counts_ptr,
                            leaf_list_ptr, leaf_counts_ptr, trunk_ptr, skip_ptr=None, trmax_ptr=None, trunk_override_ptr=None, dxoff=0, dyoff=0, xoff2=0, yoff2=0):
        """the tree draw lists of a device-resident batch, from the records the placement calls left on the device: tile_out_ptr [n] terra_tree_view_tile, all_bcube_ptr
        [n][6] floats, pine_insts_ptr / palm_insts_ptr [n][capacity] terra_tree_view_inst, inst_counts_ptr / leaf_counts_ptr [n][2] uint32, leaf_list_ptr [n][capacity]
        uint32, trunk_ptr [n][capacity] bytes; skip_ptr [n] bytes (the terrain view's not_drawn), trmax_ptr [n] floats, trunk_override_ptr [n][capacity] or None.
        view and args are host structs.  Only enqueues."""
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        self._ck(self.lib.terra_tiles_tree_view_dev(self.ctx, txy.ctypes.data, len(txy), dxoff, dyoff, xoff2, yoff2, C.byref(view), C.byref(args), stats_ptr, skip_ptr, trmax_ptr,
                                                    pine_ptr, pine_counts_ptr, capacity, trunk_override_ptr, tile_out_ptr, all_bcube_ptr, pine_insts_ptr, palm_insts_ptr,
                                                    inst_counts_ptr, leaf_list_ptr, leaf_counts_ptr, trunk_ptr))

    def tiles_scenery_view_dev(self, tile_xy, view, args, stats_ptr, objs_ptr, counts_ptr, capacity, tile_out_ptr, draw_ptr, size_scale_ptr, dist_ptr, list_ptr, list_capacity,
                               group_counts_ptr, skip_ptr=None, radius_override_ptr=None, dxoff=0, dyoff=0, xoff2=0, yoff2=0):
        """the scenery draw lists of a device-resident batch, from the records tiles_place_scenery_dev left on the device: tile_out_ptr [n] terra_scenery_view_tile,
        draw_ptr [n][capacity] uint32, size_scale_ptr / dist_ptr [n][capacity] floats, list_ptr [n][list_capacity] uint32, group_counts_ptr [n][len(SCV_GROUPS)] uint32;
        skip_ptr [n] bytes (the terrain view's not_drawn), radius_override_ptr [n][capacity] floats or None.  view and args are host structs.  Only enqueues."""
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        self._ck(self.lib.terra_tiles_scenery_view_dev(self.ctx, txy.ctypes.data, len(txy), dxoff, dyoff, xoff2, yoff2, C.byref(view), C.byref(args), stats_ptr, skip_ptr, objs_ptr,
                                                       counts_ptr, capacity, radius_override_ptr, tile_out_ptr, draw_ptr, size_scale_ptr, dist_ptr, list_ptr, list_capacity,
                                                       group_counts_ptr))

    def tiles_decid_view_dev(self, tile_xy, view, args, tree_data_ptr, num_tree_data, decid_ptr, counts_ptr, capacity, out_ptrs, skip_ptr=None, not_visible_ptr=None, dxoff=0,
                             dyoff=0, xoff2=0, yoff2=0):
        """the deciduous tree draw lists of a device-resident batch, from the records tiles_place_decid_trees_dev and tiles_edit_trees_dev keep on the device:
        tree_data_ptr [num_tree_data] terra_decid_tree_data on the device; out_ptrs: the device pointers of DECID_VIEW_OUTPUTS in that order (shapes as
        _decid_view_outputs); skip_ptr [n] bytes (the terrain view's not_drawn), not_visible_ptr [n][capacity] bytes or None.  view and args are host structs.  Only enqueues."""
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        assert len(out_ptrs) == len(self.DECID_VIEW_OUTPUTS)
        self._ck(self.lib.terra_tiles_decid_view_dev(self.ctx, txy.ctypes.data, len(txy), dxoff, dyoff, xoff2, yoff2, C.byref(view), C.byref(args), tree_data_ptr, num_tree_data,
                                                     skip_ptr, decid_ptr, counts_ptr, capacity, not_visible_ptr, *out_ptrs))

    def tiles_tree_ao_shadows_dev(self, tile_xy, list_capacity, tree_map_ptr, pine_ptr=None, pine_counts_ptr=None, pine_capacity=0, decid_ptr=None, decid_counts_ptr=None,
                                  decid_capacity=0, decid_radius_ptr=None, decid_radius_by_id_ptr=None, num_radius_by_id=0, flags_ptr=None, updated_ptr=None, trmax_ptr=None,
                                  list_counts_ptr=None, dxoff=0, dyoff=0, xoff2=0, yoff2=0):
        """the tree AO shadows of a device-resident batch, from the records the placement calls left on the device: tree_map_ptr [n][S+1][S+1][2] bytes, updated_ptr
        n bytes, trmax_ptr n floats, list_counts_ptr n uint32 (each or None).  Only enqueues."""
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        self._ck(self.lib.terra_tiles_tree_ao_shadows_dev(self.ctx, txy.ctypes.data, len(txy), dxoff, dyoff, xoff2, yoff2, pine_ptr, pine_counts_ptr, pine_capacity,
                                                          decid_ptr, decid_counts_ptr, decid_capacity, decid_radius_ptr, decid_radius_by_id_ptr, num_radius_by_id,
                                                          flags_ptr, list_capacity, tree_map_ptr, updated_ptr, trmax_ptr, list_counts_ptr))

    def tiles_edit_trees_dev(self, tile_xy, stats_ptr, pos, radius, add_trees, is_square, trmax_ptr, status_ptr, changed_ptr, pine_ptr=None, pine_counts_ptr=None,
                             pine_capacity=0, decid_ptr=None, decid_counts_ptr=None, decid_capacity=0, decid_radius_ptr=None, decid_radius_by_id_ptr=None, num_radius_by_id=0,
                             skip_ptr=None, z_ptr=None, gen_flags_ptr=None, update_bcube_ptr=None, dxoff=0, dyoff=0, xoff2=0, yoff2=0):
        """the tree brush on the device-resident records of a batch, in place: trmax_ptr n floats (in / out), status_ptr / changed_ptr n bytes, update_bcube_ptr 6 floats
        (or None).  Only enqueues; nothing is read back."""
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        self._ck(self.lib.terra_tiles_edit_trees_dev(self.ctx, txy.ctypes.data, len(txy), dxoff, dyoff, xoff2, yoff2, (C.c_float * 3)(*pos), radius, int(bool(add_trees)),
                                                     int(bool(is_square)), skip_ptr, stats_ptr, z_ptr, gen_flags_ptr, pine_ptr, pine_counts_ptr, pine_capacity, decid_ptr,
                                                     decid_counts_ptr, decid_capacity, decid_radius_ptr, decid_radius_by_id_ptr, num_radius_by_id, trmax_ptr, status_ptr,
                                                     changed_ptr, update_bcube_ptr))

    def tiles_ao_lighting_dev(self, tile_xy, z_ptr, ao_ptr):
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        self._ck(self.lib.terra_tiles_ao_lighting_dev(self.ctx, txy.ctypes.data, len(txy), z_ptr, ao_ptr))

    def voxel_fill_dev(self, ptr, nx, ny, nz, lo_pos, vsz, offset, mag, freq, rseed1, rseed2, gen_mode, zscale, normalize):
        a = lambda v: (C.c_float * 3)(*v)
        self._ck(self.lib.terra_voxel_fill_dev(self.ctx, ptr, nx, ny, nz, a(lo_pos), a(vsz), a(offset), mag, freq, rseed1, rseed2, gen_mode, zscale, normalize))

    def voxel_fill_slab_dev(self, ptr, nx, ny, nz, lo_pos, vsz, offset, mag, freq, rseed1, rseed2, gen_mode, zscale, normalize, y0, nys):
        a = lambda v: (C.c_float * 3)(*v)
        self._ck(self.lib.terra_voxel_fill_slab_dev(self.ctx, ptr, nx, ny, nz, a(lo_pos), a(vsz), a(offset), mag, freq, rseed1, rseed2, gen_mode, zscale, normalize, y0, nys))

    # ---- async generator handle (mesh_xy_grid_cache_t protocol)
    def generator(self):
        return Generator(self)


class DistributedGrid:
    """terra_dgrid: ONE array whose strips live on several GPUs, mapped back to back in this rank's address space (HIP virtual memory management).
    rank r: g = DistributedGrid(terra, strip_bytes, r); fd = g.export_fd() -> peers; g.import_fd(j, fd_j) for every other strip; ptr = g.map()"""

    def __init__(self, terra, strip_bytes, local_strip):
        self.t = terra
        arr = (_sz * len(strip_bytes))(*[int(b) for b in strip_bytes])
        h = _vp()
        terra._ck(terra.lib.terra_dgrid_create(terra.ctx, len(strip_bytes), arr, local_strip, C.byref(h)))
        self.h, self.strip_bytes, self.local, self.ptr = h, [int(b) for b in strip_bytes], local_strip, None

    @staticmethod
    def granularity(terra):
        return int(terra.lib.terra_dgrid_granularity(terra.ctx))

    def export_fd(self):
        fd = _i32()
        self.t._ck(self.t.lib.terra_dgrid_export_fd(self.h, C.byref(fd)))
        return fd.value

    def import_fd(self, strip, fd):
        self.t._ck(self.t.lib.terra_dgrid_import_fd(self.h, strip, fd))

    def map(self):
        p = _vp()
        self.t._ck(self.t.lib.terra_dgrid_map(self.h, C.byref(p)))
        self.ptr = p.value
        return self.ptr

    def strip_ptr(self, i):
        return self.ptr + sum(self.strip_bytes[:i])

    def destroy(self):
        if self.h:
            self.t.lib.terra_dgrid_destroy(self.h)
            self.h = None


class TerraMulti:
    """terra_multi: several contexts (one per entry of `devices`, indices may repeat) driven from this process, each by its own host thread inside a call."""

    def __init__(self, devices, lib_path=None):
        self.lib = load_library(lib_path)
        m = _vp()
        arr = (_i32 * len(devices))(*devices)
        rc = self.lib.terra_multi_create(C.byref(m), arr, len(devices))
        if rc != 0:
            raise TerraError(rc, self.lib.terra_last_error().decode())
        self.m = m
        self.n = len(devices)
        self.ctxs = []
        for i in range(self.n):  # borrowed contexts: the plumbing (alloc / upload / download) of Terra works on them, close() is the multi handle's
            t = Terra.__new__(Terra)
            t.lib, t.ctx = self.lib, _vp(self.lib.terra_multi_ctx(self.m, i))
            t.close = lambda: None
            self.ctxs.append(t)

    def close(self):
        if getattr(self, "m", None):
            for t in self.ctxs:
                t.ctx = None
            self.lib.terra_multi_destroy(self.m)
            self.m = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc < 0:
            raise TerraError(rc, self.lib.terra_last_error().decode())
        return rc

    def partition(self, n_units, part):
        a, b = _u32(), _u32()
        self.lib.terra_multi_partition(n_units, self.n, part, C.byref(a), C.byref(b))
        return a.value, b.value

    def init_scene(self, cfg):
        self._ck(self.lib.terra_multi_init_scene(self.m, C.byref(cfg)))
        return self.ctxs[0].state()

    def synchronize(self): self._ck(self.lib.terra_multi_synchronize(self.m))

    def dgrid_create(self, strip_bytes):
        """strip i on context i's device, all mapped back to back: (handle, device pointer valid on every context's device); free with dgrid_destroy"""
        arr = (_sz * self.n)(*[int(b) for b in strip_bytes])
        h, p = _vp(), _vp()
        self._ck(self.lib.terra_multi_dgrid_create(self.m, arr, C.byref(h), C.byref(p)))
        return h, p.value

    def dgrid_destroy(self, h): self.lib.terra_dgrid_destroy(h)

    def tiles_create_zvals(self, tile_xy, iters_tt=0):
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        n = len(txy)
        s = _u32()
        self._ck(self.lib.terra_tile_size(self.lib.terra_multi_ctx(self.m, 0), C.byref(s)))  # (every context has the same scene)
        S = s.value
        z = np.empty((n, S + 2, S + 2), np.float32); st = (TileStats * n)(); nm = np.empty((n, S + 1, S + 1, 4), np.uint8); mnz = np.empty(n, np.float32)
        self._ck(self.lib.terra_multi_tiles_create_zvals(self.m, txy.ctypes.data, n, iters_tt, z.ctypes.data, C.addressof(st), nm.ctypes.data, mnz.ctypes.data))
        return z, st, nm, mnz

    def tiles_create_zvals_dev(self, tile_xy, iters_tt, z_ptrs, stats_ptrs=None, normals_ptrs=None, mnz_ptrs=None):
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        arr = lambda ps: None if ps is None else (_vp * self.n)(*ps)
        self._ck(self.lib.terra_multi_tiles_create_zvals_dev(self.m, txy.ctypes.data, len(txy), iters_tt, arr(z_ptrs), arr(stats_ptrs), arr(normals_ptrs), arr(mnz_ptrs)))

    def gen_grid_rows_dev(self, ptrs, x0, y0, dx, dy, nx, ny, flags=GEN_GLACIATE, min_start_sin=0):
        mn, mx = C.c_float(), C.c_float()
        self._ck(self.lib.terra_multi_gen_grid_rows_dev(self.m, x0, y0, dx, dy, nx, ny, flags, min_start_sin, (_vp * self.n)(*ptrs), C.byref(mn), C.byref(mx)))
        return mn.value, mx.value

    def voxel_fill_dev(self, ptrs, nx, ny, nz, lo_pos, vsz, offset, mag, freq, rseed1, rseed2, gen_mode, zscale, normalize):
        a = lambda v: (C.c_float * 3)(*v)
        self._ck(self.lib.terra_multi_voxel_fill_dev(self.m, (_vp * self.n)(*ptrs), nx, ny, nz, a(lo_pos), a(vsz), a(offset), mag, freq, rseed1, rseed2, gen_mode, zscale, normalize))

    def tiles_mesh_shadows(self, tile_xy, zvals, light_pos):
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        n = len(txy)
        z = np.ascontiguousarray(zvals, np.float32).reshape(n, 130, 130)
        sm = np.empty((n, 130, 130), np.uint8)
        self._ck(self.lib.terra_multi_tiles_mesh_shadows(self.m, txy.ctypes.data, n, z.ctypes.data, (C.c_float * 3)(*light_pos), sm.ctypes.data))
        return sm

    def shadow_layout(self, tile_xy, light_pos):
        """where the device-resident mesh-shadow pass wants the tiles: (ctx_of_tile, pos_in_ctx, tiles_per_ctx)"""
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        n = len(txy)
        a, b, c = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(self.n, np.uint32)
        self._ck(self.lib.terra_multi_shadow_layout(self.m, txy.ctypes.data, n, (C.c_float * 3)(*light_pos), a.ctypes.data, b.ctypes.data, c.ctypes.data))
        return a, b, c

    def tiles_mesh_shadows_dev(self, tile_xy, z_ptrs, light_pos, smask_ptrs):
        """z_ptrs[s] / smask_ptrs[s]: context s's strip in the order of shadow_layout, on its device"""
        txy = np.ascontiguousarray(tile_xy, np.int32).reshape(-1, 2)
        zp = (_vp * self.n)(*z_ptrs); sp = (_vp * self.n)(*smask_ptrs)
        self._ck(self.lib.terra_multi_tiles_mesh_shadows_dev(self.m, txy.ctypes.data, len(txy), zp, (C.c_float * 3)(*light_pos), sp))

    def foreach(self, fn):
        """fn(Terra, index) -> int on every context's host thread at once (the callback re-enters Python: the calls serialise on the GIL except inside the library)"""
        cb_t = C.CFUNCTYPE(C.c_int, _vp, _u32, _vp)
        def tramp(ctx, index, _user):
            try:
                r = fn(self.ctxs[index], index)
                return 0 if r is None else int(r)
            except Exception:  # noqa: BLE001
                return -2
        cb = cb_t(tramp)
        self._ck(self.lib.terra_multi_foreach(self.m, C.cast(cb, _vp), None))


class Generator:
    def __init__(self, terra):
        self.t = terra
        g = _vp()
        terra._ck(terra.lib.terra_gen_create(terra.ctx, C.byref(g)))
        self.g = g
        self.shape = None

    def build_arrays(self, x0, y0, dx, dy, nx, ny, flags=0, min_start_sin=0):
        self.shape = (ny, nx)
        return self.t._ck(self.t.lib.terra_gen_build_arrays(self.g, x0, y0, dx, dy, nx, ny, flags, min_start_sin))

    def enable_glaciate(self): self.t._ck(self.t.lib.terra_gen_enable_glaciate(self.g))
    def is_running(self): return bool(self.t.lib.terra_gen_is_running(self.g))
    def eval_index(self, x, y, min_start_sin=0, use_cache=True): return self.t.lib.terra_gen_eval_index(self.g, x, y, min_start_sin, 1 if use_cache else 0)

    def collect(self):
        out = np.empty(self.shape, np.float32)
        self.t._ck(self.t.lib.terra_gen_collect(self.g, out.ctypes.data))
        return out

    def close(self):
        if self.g:
            self.t.lib.terra_gen_destroy(self.g)
            self.g = None
