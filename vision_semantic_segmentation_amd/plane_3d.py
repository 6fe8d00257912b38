"""The ground plane a x + b y + c z + d = 0 of the reference (src/plane_3d.py), as far as the convex-hull back-projection needs
it: construction with the reference's normalisation, the two distance functions and the two ray intersections.  Host-side float64
with the reference's order of operations.  Plane fitting, the weighted cost, rotation and plotting are not built.
"""
import numpy as np


class Plane3D(object):
    def __init__(self, a=0., b=0., c=0., d=0.):
        self.a, self.b, self.c, self.d = float(a), float(b), float(c), float(d)
        self.normalize()

    @classmethod
    def create_plane_from_list(cls, param):
        """src/plane_3d.py:27-29"""
        return cls(param[0], param[1], param[2], param[3])

    def normalize(self):
        """src/plane_3d.py:98-107: unit normal, signed so that c >= 0; ``param`` is the [4, 1] column (a, b, c, d).  An all-zero
        normal is left as it is and has no ``param`` (the reference prints an error and goes on)."""
        length = np.sqrt(self.a**2 + self.b**2 + self.c**2)
        if length == 0:
            return
        if self.c < 0:
            length = -1 * length
        self.a, self.b, self.c, self.d = self.a / length, self.b / length, self.c / length, self.d / length
        self.param = np.array([[self.a, self.b, self.c, self.d]]).T

    def _offsets(self, data):
        return (np.matmul(data, self.param[0:3, :]) + self.d).reshape([-1])

    def distance_to_plane(self, data):
        """src/plane_3d.py:82-88: data [n, 3] -> unsigned distances [n] (inf for a degenerate normal)."""
        length = np.sqrt(self.a**2 + self.b**2 + self.c**2)
        if length > 1e-3:
            return np.abs(self._offsets(data)) / length
        return np.ones((data.shape[0])) * np.inf

    def distance_to_plane_signed(self, data):
        """src/plane_3d.py:90-96"""
        length = np.sqrt(self.a**2 + self.b**2 + self.c**2)
        if length > 1e-3:
            return self._offsets(data) / length
        return self._offsets(data) * np.inf

    def plane_ray_intersection(self, d, C):
        """src/plane_3d.py:145-148: the point C + lam d of the plane; d, C [3, 1]."""
        normal = self.param[0:3, :].T
        lam = (-1 * np.matmul(normal, C) - self.d) / (np.matmul(normal, d))
        return d * lam + C

    def plane_ray_intersection_vec(self, d, C):
        """src/plane_3d.py:150-154: d [3, n] directions through the common point C [3, 1] -> [3, n] intersections."""
        normal = np.array([[self.a, self.b, self.c]])
        k = (-self.d - np.matmul(normal, C).item()) / np.matmul(normal, d)
        return k * d + C
