"""hash_to_curve for Pallas and Vesta in Python integers and hashlib.blake2b: the model csrc/blake2b.h, csrc/hashtocurve.h and
csrc/hashtocurve.hip are tested against (DESIGN.md "Params::new on the device").

    hash_to_field   RFC 9380 section 5.3.1 expand_message_xmd over BLAKE2b-512 (block 128 bytes, digest 64), two elements of 64 bytes each,
                    DST = prefix || "-" || curve || "_XMD:BLAKE2b_SSWU_RO_"
    map_to_curve    RFC 9380 section 6.6.2, simplified SWU onto the iso-curve y^2 = x^3 + A x + 1265 with Z = -13
    iso_map         the 3-isogeny to y^2 = x^3 + 5, DERIVED here from A and 1265 by Velu's formulas -- no constant of it is typed in
    hash_to_curve   iso_map(swu(u0) + swu(u1)), cofactor 1

What is pinned by what: the hash by hashlib, the group orders and the isogeny by the integer checks of tests/test_hashtocurve_host.py.  That
pasta_curves 0.4 / halo2_proofs 0.2.0 use this very DST layout, these message bytes and this isogeny (and not its negative) is recalled, not
pinned: tests/golden/hash_to_curve_kat.json holds the values to compare the day the Rust crates are at hand.

Points are (x, y) tuples of canonical integers, None the identity."""
import hashlib

P_MOD = 0x40000000000000000000000000000000224698FC094CF91B992D30ED00000001
Q_MOD = 0x40000000000000000000000000000000224698FC0994A8DD8C46EB2100000001
ISO_B = 1265
Z = -13
CURVE_B = 5
MAX_PREFIX = 128


class IsoCurve:
    """One curve's map: base field modulus m, group order, iso-curve coefficient A, and everything derived from them."""

    def __init__(self, name, m, order, a):
        self.name, self.m, self.order, self.a, self.b = name, m, order, a, ISO_B
        self.z = Z % m
        # kernel abscissa of the 3-isogeny: x0^2 = -3 A / 10, and the 3-division polynomial vanishes at it
        r = sqrt_mod(-3 * a * pow(10, -1, m) % m, m)
        assert r is not None, "-3A/10 is not a square: no rational 3-isogeny of this shape"
        roots = [x for x in (r, m - r) if self.div3(x) == 0]
        assert len(roots) == 1, "exactly one of the two square roots is the kernel's abscissa"
        self.x0 = roots[0]
        # Velu: t = 2 (3 x0^2 + A), u = 4 (x0^3 + A x0 + B)
        self.t = 2 * (3 * self.x0 * self.x0 + a) % m
        self.u = 4 * (self.x0 ** 3 + a * self.x0 + self.b) % m
        # codomain y^2 = x^3 + (A - 5 t) x + (B - 7 (u + x0 t)): must be y^2 = x^3 + 5 * 3^6
        assert (a - 5 * self.t) % m == 0 and (self.b - 7 * (self.u + self.x0 * self.t)) % m == 3645
        # the square root the device's fixed-schedule chain returns for a non-square a is sqrt(a g), g the 2^32-th root of unity of
        # fieldsqrt.h; the second candidate's y is then theta u^3 sqrt(a g) / den with theta = Z sqrt(Z / g)
        self.g = pow(5, (m - 1) >> 32, m)
        s = sqrt_mod(self.z * pow(self.g, -1, m) % m, m)
        assert s is not None
        self.theta = self.z * min(s, m - s) % m
        self.iso = self.iso_polynomials()

    def div3(self, x):
        return (3 * x ** 4 + 6 * self.a * x * x + 12 * self.b * x - self.a * self.a) % self.m

    def iso_polynomials(self):
        """The same map as rational functions, the shape of pasta_curves' table of 13 constants (highest degree first):
        X = x_num(x) / x_den(x), Y = y y_num(x) / y_den(x), x_den and y_den monic."""
        m, x0, t, u = self.m, self.x0, self.t, self.u
        i9, i27 = pow(9, -1, m), pow(27, -1, m)
        # X = (x d^2 + t d + u) / (9 d^2), d = x - x0
        x_num = [1, -2 * x0, x0 * x0 + t, u - t * x0]
        x_den = [1, -2 * x0, x0 * x0]
        # Y = y (d^3 - t d - 2 u) / (27 d^3)
        y_num = [1, -3 * x0, 3 * x0 * x0 - t, -x0 ** 3 + t * x0 - 2 * u]
        y_den = [1, -3 * x0, 3 * x0 * x0, -x0 ** 3]
        return {"x_num": [c * i9 % m for c in x_num], "x_den": [c % m for c in x_den],
                "y_num": [c * i27 % m for c in y_num], "y_den": [c % m for c in y_den]}

    # ---- the iso-curve's group ------------------------------------------------------------------------------------------------------
    def on_iso(self, p):
        return p is None or (p[1] * p[1] - (p[0] ** 3 + self.a * p[0] + self.b)) % self.m == 0

    def on_curve(self, p):
        return p is None or (p[1] * p[1] - (p[0] ** 3 + CURVE_B)) % self.m == 0

    def add(self, p, q, a=None):
        """Affine addition on y^2 = x^3 + a x + b (a defaults to the iso-curve's A; a = 0 is the target curve)."""
        a = self.a if a is None else a
        m = self.m
        if p is None: return q
        if q is None: return p
        if p[0] == q[0]:
            if (p[1] + q[1]) % m == 0: return None
            lam = (3 * p[0] * p[0] + a) * pow(2 * p[1], -1, m) % m
        else:
            lam = (q[1] - p[1]) * pow(q[0] - p[0], -1, m) % m
        x = (lam * lam - p[0] - q[0]) % m
        return (x, (lam * (p[0] - x) - p[1]) % m)

    def mul(self, k, p, a=None):
        acc = None
        while k:
            if k & 1: acc = self.add(acc, p, a)
            p = self.add(p, p, a)
            k >>= 1
        return acc

    # ---- RFC 9380 -------------------------------------------------------------------------------------------------------------------
    def sgn0(self, x):
        return x % self.m & 1

    def swu(self, u):
        """map_to_curve_simple_swu, section 6.6.2 as written (with inversions): a point of the iso-curve."""
        m, a, b, z = self.m, self.a, self.b, self.z
        u %= m
        tv1 = (z * z * pow(u, 4, m) + z * u * u) % m
        if tv1 == 0:
            x1 = b * pow(z * a, -1, m) % m
        else:
            x1 = -b * pow(a, -1, m) * (1 + pow(tv1, -1, m)) % m
        gx1 = (x1 ** 3 + a * x1 + b) % m
        x2 = z * u * u * x1 % m
        gx2 = (x2 ** 3 + a * x2 + b) % m
        y1 = sqrt_mod(gx1, m)
        if y1 is not None:
            x, y = x1, y1
        else:
            x, y = x2, sqrt_mod(gx2, m)
            assert y is not None
        if self.sgn0(u) != self.sgn0(y):
            y = m - y
        return (x, y)

    def gx1_is_square(self, u):
        m, a, b, z = self.m, self.a, self.b, self.z
        tv1 = (z * z * pow(u, 4, m) + z * u * u) % m
        x1 = b * pow(z * a, -1, m) % m if tv1 == 0 else -b * pow(a, -1, m) * (1 + pow(tv1, -1, m)) % m
        return sqrt_mod((x1 ** 3 + a * x1 + b) % m, m) is not None

    def iso_map(self, p):
        """Velu's form; the identity and the kernel's points (x = x0) go to the identity."""
        if p is None or p[0] == self.x0: return None
        m = self.m
        d = (p[0] - self.x0) % m
        di = pow(d, -1, m)
        X = (p[0] + self.t * di + self.u * di * di) % m
        Y = p[1] * (1 - self.t * di * di - 2 * self.u * di ** 3) % m
        return (X * pow(9, -1, m) % m, Y * pow(27, -1, m) % m)

    def iso_map_polynomial(self, p):
        if p is None: return None
        m, c = self.m, self.iso
        ev = lambda cs: sum(k * pow(p[0], len(cs) - 1 - i, m) for i, k in enumerate(cs)) % m
        xd, yd = ev(c["x_den"]), ev(c["y_den"])
        if xd == 0 or yd == 0: return None
        return (ev(c["x_num"]) * pow(xd, -1, m) % m, p[1] * ev(c["y_num"]) * pow(yd, -1, m) % m)

    def dst(self, prefix: bytes) -> bytes:
        return prefix + b"-" + self.name.encode() + b"_XMD:BLAKE2b_SSWU_RO_"

    def hash_to_field(self, prefix: bytes, msg: bytes):
        assert len(prefix) <= MAX_PREFIX
        dst = self.dst(prefix)
        dstp = dst + bytes([len(dst)])
        H = lambda b: hashlib.blake2b(b, digest_size=64, person=bytes(16)).digest()
        b0 = H(bytes(128) + msg + bytes([0, 128, 0]) + dstp)
        b1 = H(b0 + b"\x01" + dstp)
        b2 = H(bytes(x ^ y for x, y in zip(b0, b1)) + b"\x02" + dstp)
        return [int.from_bytes(b1, "big") % self.m, int.from_bytes(b2, "big") % self.m]

    def map_sum(self, us):
        """iso_map(sum swu(u)): the device's trh_map_to_curve_dev record."""
        acc = None
        for u in us:
            acc = self.add(acc, self.swu(u))
        return self.iso_map(acc)

    def hash_to_curve(self, prefix: bytes, msg: bytes):
        return self.map_sum(self.hash_to_field(prefix, msg))


def sqrt_mod(a, m):
    """A square root of a mod the prime m (Tonelli-Shanks), None for a non-square."""
    a %= m
    if a == 0: return 0
    if pow(a, (m - 1) // 2, m) != 1: return None
    s, q = 0, m - 1
    while q % 2 == 0: s, q = s + 1, q // 2
    z = 2
    while pow(z, (m - 1) // 2, m) == 1: z += 1
    c, x, t, mm = pow(z, q, m), pow(a, (q + 1) // 2, m), pow(a, q, m), s
    while t != 1:
        i, t2 = 0, t
        while t2 != 1: t2, i = t2 * t2 % m, i + 1
        bb = pow(c, 1 << (mm - i - 1), m)
        x, c, mm = x * bb % m, bb * bb % m, i
        t = t * c % m
    return x


PALLAS = IsoCurve("pallas", P_MOD, Q_MOD, 0x18354a2eb0ea8c9c49be2d7258370742b74134581a27a59f92bb4b0b657a014b)
VESTA = IsoCurve("vesta", Q_MOD, P_MOD, 0x267f9b2ee592271a81639c4d96f787739673928c7d01b212c515ad7242eaa6b1)
CURVES = {"pallas": PALLAS, "vesta": VESTA}

HALO2_PREFIX = b"Halo2-Parameters"


def params_g(curve: str, i: int):
    return CURVES[curve].hash_to_curve(HALO2_PREFIX, b"\x00" + i.to_bytes(4, "little"))


def params_w(curve: str):
    return CURVES[curve].hash_to_curve(HALO2_PREFIX, b"\x01")


def params_u(curve: str):
    return CURVES[curve].hash_to_curve(HALO2_PREFIX, b"\x02")


def point_limbs(m, p):
    """The 64-byte affine POD as eight u64 (Montgomery, R = 2^256); the identity is all zero."""
    if p is None: return [0] * 8
    out = []
    for v in p:
        v = v * (1 << 256) % m
        out += [(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)]
    return out
