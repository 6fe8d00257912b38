"""The ground plane a x + b y + c z + d = 0 of the reference (src/plane_3d.py): construction with the reference's normalisation,
the minimal three-point fit, the x-distance-weighted cost, the two distance functions, rotation, the normal's angles and the two
ray intersections.  Host-side float64 with the reference's order of operations.  Plotting (``vis``) is not built, and
``fit(method="least_square")`` is as unimplemented as in the reference (ground_plane.plane_from_moments has the refit).
"""
import numpy as np


def default_weight():
    """src/plane_3d.py:19 -- the constructor's default weight (a fresh dict per call; the reference shares one)."""
    return {'method': "x norm", 'param': {'x0': 0.0, 'norm': 1}}


class Plane3D(object):
    def __init__(self, a=0., b=0., c=0., d=0., weight=None):
        self.a, self.b, self.c, self.d = float(a), float(b), float(c), float(d)
        self.weight = default_weight() if weight is None else weight
        self.normalize()

    @classmethod
    def create_plane_from_list(cls, param):
        """src/plane_3d.py:27-29"""
        return cls(param[0], param[1], param[2], param[3])

    @classmethod
    def create_plane_from_vectors_and_point(cls, vec1, vec2, pt1):
        """src/plane_3d.py:31-42: the plane through pt1 that holds the directions vec1 and vec2 (each an array of 3)."""
        pt2 = vec1 / np.linalg.norm(vec1) + pt1
        pt3 = vec2 / np.linalg.norm(vec2) + pt1
        pts = np.vstack([pt1, pt2, pt3])
        return cls.fit(pts, method="min")

    @classmethod
    def fit(cls, data, method="least_square", weight=None):
        """src/plane_3d.py:44-63: method "min" = the plane through the three rows of data [3, 3]; data[0] == data[1] or another
        number of rows raises ValueError (the reference prints and calls exit()).  Every other method is NotImplementedError."""
        if method == "min":
            if len(data) == 3 and not np.all(data[0, :] - data[1, :] == 0):
                a = (data[0, 1] - data[1, 1]) * (data[2, 2] - data[1, 2]) - (data[2, 1] - data[1, 1]) * (data[0, 2] - data[1, 2])
                b = (data[0, 2] - data[1, 2]) * (data[2, 0] - data[1, 0]) - (data[2, 2] - data[1, 2]) * (data[0, 0] - data[1, 0])
                c = (data[0, 0] - data[1, 0]) * (data[2, 1] - data[1, 1]) - (data[2, 0] - data[1, 0]) * (data[0, 1] - data[1, 1])
                d = -a * data[1, 0] - b * data[1, 1] - c * data[1, 2]
            else:
                raise ValueError("incorrect data: the minimal model needs three points, the first two distinct")
        else:
            raise NotImplementedError
        if weight is None:
            return cls(a, b, c, d)
        return cls(a, b, c, d, weight=weight)

    def eval(self, data):
        """src/plane_3d.py:65-80: data [n, 3] -> the point-to-plane distances [n], for "x norm" scaled by
        (1 / (|x - x0|^norm + 1)) / its maximum over data, so that points far along x count less."""
        if self.weight['method'] == "x norm":
            if self.weight['param']['norm'] == 1:
                x_norm = np.abs(data[:, 0] - self.weight['param']['x0'])
            elif self.weight['param']['norm'] == 2:
                x_norm = (data[:, 0] - self.weight['param']['x0'])**2
            else:
                raise NotImplementedError
            x_distance_recip = 1 / (x_norm + 1)
            x_distance_weight = x_distance_recip / np.max(x_distance_recip)
            cost = self.distance_to_plane(data) * x_distance_weight
        elif self.weight['method'] == "none":
            cost = self.distance_to_plane(data)
        else:
            raise NotImplementedError
        return cost

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

    def rotate_around_axis(self, axis, angle):
        """src/plane_3d.py:109-116: turns the normal about "y" by angle (radians); any other axis only refreshes ``param``."""
        if axis == "y":
            norm = np.sqrt(self.a**2 + self.c**2)
            theta = np.arctan2(self.c, self.a)
            theta_2 = theta + angle
            self.a, self.c = np.cos(theta_2) * norm, np.sin(theta_2) * norm
        self.param = np.array([[self.a, self.b, self.c, self.d]]).T

    def normal_angle_to_vector(self, vector):
        """src/plane_3d.py:118-129: the angle between the plane's normal and vector (3 values)."""
        vector = vector.reshape([3, 1]) / np.linalg.norm(vector)
        self.normalize()
        angle = np.arccos(np.matmul(vector.T, self.param[0:3, :]))
        return angle[0, 0]

    def normal_angle_to_vector_xz(self, vector):
        """src/plane_3d.py:131-143: the same angle between the projections onto the xz plane."""
        vector = vector.reshape([3, 1])
        inner = (vector[0, 0] * self.a + vector[2, 0] * self.c)
        scaling = np.sqrt(vector[0, 0]**2 + vector[2, 0]**2) * np.sqrt(self.a**2 + self.c**2)
        return np.arccos(inner / scaling)

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
