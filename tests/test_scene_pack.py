"""pack_scene (izpi_amd/csrc/scene_pack.cpp): the host half of izpi_gpu_upload_scene, checked
without a GPU in a stand-alone program under AddressSanitizer and UBSan."""
import subprocess
from pathlib import Path

import pytest

from izpi_amd import _native as N

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "izpi_amd" / "csrc"

STRUCTURE = ["stack", "refs", "leaves", "contains", "rows", "mk", "lights", "tex", "slots"]
FULL = dict(quantized=0, leaf_shortcut=1, nan_free_bounds=1, time_free=1, no_pathlen=0, tri_only=0, mat_ok_rgb=1,
            mat_ok_spectral=1, basic_materials=0, matset=15, const_albedo=0, any_uv=1)
BASIC = dict(quantized=0, leaf_shortcut=1, nan_free_bounds=1, time_free=1, no_pathlen=1, tri_only=1, mat_ok_rgb=1,
             mat_ok_spectral=0, basic_materials=1, matset=0, const_albedo=1, any_uv=0)
# valid descriptors: the flags, and whether the program compared every record with the descriptor
VALID = {
    "full": (FULL, True),
    "full_quantized": (dict(FULL, quantized=1), True),
    "basic": (BASIC, True),
    "basic_quantized": (dict(BASIC, quantized=1), True),
    "moving_sphere": (dict(FULL, time_free=0), True),
    "camera_before_sphere": (dict(FULL, time_free=0), True),
    "nan_bound": (dict(FULL, nan_free_bounds=0, leaf_shortcut=0), False),  # (NaN != NaN: the leaf's box differs too)
    "leaf_box_changed": (dict(FULL, leaf_shortcut=0), False),
    "leaf_box_changed_quantized": (dict(FULL, quantized=1, leaf_shortcut=1), False),  # re-test box = decoded parent slot
    "no_rgb_albedo": (dict(FULL, mat_ok_rgb=0), True),
    "no_spectral_albedo": (dict(FULL, mat_ok_spectral=0), True),
}
# every error return of the packer, each reached by one mutation of the full scene
ERRORS = {
    "leaf_second_slot": (N.IZPI_ERR_INVALID, "leaf node with more than one slot"),
    "leaf_range": (N.IZPI_ERR_INVALID, "leaf primitive range out of bounds"),
    "leaf_count_8": (N.IZPI_ERR_UNSUPPORTED, "leaf too large for the leaf-ref encoding"),
    "inner_prim_slot": (N.IZPI_ERR_INVALID, "inner node with a primitive slot"),
    "child_index": (N.IZPI_ERR_INVALID, "child index out of bounds"),
    "not_preorder": (N.IZPI_ERR_INVALID, "BVH4 nodes not in pre-order"),
    "triangle_ref": (N.IZPI_ERR_INVALID, "triangle ref out of range"),
    "sphere_ref": (N.IZPI_ERR_INVALID, "sphere ref out of range"),
    "light_triangle_ref": (N.IZPI_ERR_INVALID, "light triangle out of range"),
    "light_sphere_ref": (N.IZPI_ERR_INVALID, "light sphere out of range"),
    "normal_mapped_light": (N.IZPI_ERR_UNSUPPORTED, "normal-mapped light"),
    "texture_index": (N.IZPI_ERR_INVALID, "texture index out of range"),
    "spectral_image_in_rgb_slot": (N.IZPI_ERR_INVALID, "SpectralImage outside a spectral albedo"),
    "spectral_image_on_metal": (N.IZPI_ERR_INVALID, "SpectralImage outside a spectral albedo"),
    "material_kind": (N.IZPI_ERR_INVALID, "unknown material kind"),
    "material_index_bvh": (N.IZPI_ERR_INVALID, "material index out of range"),
    "material_index_light": (N.IZPI_ERR_INVALID, "material index out of range"),  # read out of bounds before
    "normal_map_without_tangents": (N.IZPI_ERR_INVALID, "a PBR normal map needs the triangles' tangents and bitangents"),
    "image_range": (N.IZPI_ERR_INVALID, "image texture outside the texel array"),
    "spd_range": (N.IZPI_ERR_INVALID, "SPD range out of bounds"),
}


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    exe = tmp_path_factory.mktemp("scene_pack") / "scene_pack_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", str(exe), str(ROOT / "tests" / "scene_pack_check.cpp"), str(CSRC / "scene_pack.cpp"),
                    str(CSRC / "host_scene.cpp")], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr[-3000:]  # a sanitizer report ends the program
    out = {}
    for line in run.stdout.splitlines():
        name, rc, err, fields = line.split("|")
        out[name] = (int(rc), err, {k: int(v) for k, v in (f.split("=") for f in fields.split())})
    return out


def test_every_case_ran(rows):
    assert sorted(rows) == sorted([*VALID, *ERRORS])


@pytest.mark.parametrize("name", sorted(VALID))
def test_valid_descriptor_packs(rows, name):
    rc, err, f = rows[name]
    flags, compared = VALID[name]
    assert (rc, err) == (N.IZPI_OK, "")
    assert {k: f[k] for k in flags} == flags
    if compared:
        assert {k: f[k] for k in STRUCTURE} == dict.fromkeys(STRUCTURE, 1)
    if flags["any_uv"]:
        # the gray image (3 texels) at one double per texel, the RGBA run (2 x 2) 32-B aligned
        # behind it, then the SpectralImage's own copy of those texels
        assert (f["gray_at"], f["rgba_at"], f["texels"]) == (0, 4, 36)
    else:
        assert f["texels"] == 1


def test_every_flag_takes_both_values():
    for k in FULL:
        assert {flags[k] for flags, _ in VALID.values()} >= ({0, 15} if k == "matset" else {0, 1}), k


@pytest.mark.parametrize("name", sorted(ERRORS))
def test_bad_descriptor_is_refused(rows, name):
    rc, err, _ = rows[name]
    assert (rc, err) == ERRORS[name]
