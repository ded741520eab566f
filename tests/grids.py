"""The grids of the SDF field and mesh tests (a helper, not a test)."""
import ctypes as C

import numpy as np

import sdf_mesh_model as MM

F32 = np.float32

# object, origin, step, dims, iTime, vertices, quads, Euler characteristic: grids on which
# the model's mesh was checked to be closed (coarser ones over the thin capsule are not)
GRIDS = [("sphere", (11.05, -4.1, -14.05), 0.9, (10, 10, 10), 0.0, 194, 192, 2),
         ("blend", (-9.6, -4.2, -14.3), 0.6, (17, 15, 16), 1.0, 460, 458, 2),
         ("capsule", (-7.2, -4.05, -32.1), 0.41, (16, 20, 16), 0.0, 402, 400, 2),
         ("torus", (-8.6, -3.55, 9.05), 0.29, (26, 26, 8), 1.0, 774, 774, 0),
         ("torus_coarse", (-8.6, -3.55, 9.05), 0.45, (17, 17, 6), 1.0, 328, 328, 0)]


def desc(rm, origin, step, dims):
    return rm.rm_sdf_grid_desc((C.c_float * 3)(*origin), (C.c_float * 3)(*step), (C.c_int32 * 3)(*dims))


def step3(step):
    return (step,) * 3


def grid_points(origin, step, dims):
    """The grid's coordinates in float32: one multiply, then one add per axis; x fastest."""
    ax = MM.coords(origin, step, dims)
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return np.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], axis=1).astype(F32)
