"""Array edits of the fixture scenes for the shading gather's tests (rt_path.h shade_pre,
RT_SHADE_GATHER): which of a mesh's four texture slots (base, normal, metallic-roughness,
emission) are present, and what they point at.  Shared by tests/test_gpu_shade_gather.py (GPU
against the CPU oracle) and tests/test_shade_gather_host.py (the addressing proof on the CPU)."""
import numpy as np

EMISSION = np.array([0.5, 0.25, 1.0], np.float32)   # emission factor of a mesh whose emission slot is live


def _with_slots(base, mesh_tex):
    a = dict(base)
    a["mesh_tex"] = np.ascontiguousarray(mesh_tex, np.int32)
    a["mesh_f"] = np.asarray(base["mesh_f"], np.float32).copy()
    a["mesh_f"][a["mesh_tex"][:, 3] >= 0, 3:6] = EMISSION
    return a


def deal16(base):
    """Mesh m gets subset m % 16 of the four slots (bit k of the subset: slot k present), so
    meshes next to each other differ in every slot; a present slot keeps the mesh's own texture
    or, where it had none (the emission slot), takes one dealt from the scene's textures."""
    mt = np.asarray(base["mesh_tex"], np.int32)
    n_tex = len(base["tex_info"])
    out = np.full_like(mt, -1)
    for m in range(len(mt)):
        for k in range(4):
            if (m % 16) >> k & 1:
                out[m, k] = mt[m, k] if mt[m, k] >= 0 else (5 * m + 7 * k) % n_tex
    return _with_slots(base, out)


def shared(base):
    """Even meshes: one texture in all four slots; odd meshes: the last texture in all four."""
    n, n_tex = len(base["mesh_tex"]), len(base["tex_info"])
    out = np.empty((n, 4), np.int32)
    for m in range(n):
        out[m, :] = (3 * m) % n_tex if m % 2 == 0 else n_tex - 1
    return _with_slots(base, out)


def no_normal_maps(base):
    """Textures, but no normal map anywhere (no shaded hit reads tri_tan); every second mesh
    also has an emission texture."""
    out = np.asarray(base["mesh_tex"], np.int32).copy()
    out[:, 1] = -1
    out[::2, 3] = out[::2, 0]
    return _with_slots(base, out)


def single_1x1(base):
    """The scene's only texture is one texel, dealt over the slots as deal16 does."""
    a = deal16(base)
    a["mesh_tex"] = np.where(a["mesh_tex"] >= 0, 0, -1).astype(np.int32)
    a["tex_info"] = np.array([[0, 1, 1, 4]], np.uint32)
    a["texels"] = np.array([200, 90, 40, 255], np.uint8)
    return a


def tables_blob(arrays):
    """The material tables of a scene as tests/native/shade_gather_host.cpp reads them."""
    mf = np.ascontiguousarray(arrays["mesh_f"], np.float32).reshape(-1, 12)
    mt = np.ascontiguousarray(arrays["mesh_tex"], np.int32).reshape(-1, 4)
    ti = np.ascontiguousarray(arrays["tex_info"], np.uint32).reshape(-1, 4)
    tx = np.ascontiguousarray(arrays["texels"], np.uint8).reshape(-1)
    assert len(mf) == len(mt) and len(tx) % 4 == 0
    return np.array([len(mf), len(ti), len(tx) // 4], np.uint32).tobytes() + mf.tobytes() + mt.tobytes() + ti.tobytes() + tx.tobytes()
