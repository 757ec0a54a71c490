"""The reference of the project tests (include/linne_amd.h LINNEAmd_ProjectWindowsDevice): numpy int64 frames @ basis.T over the decoded
samples with zero halos, then the shift, the clip and the F32 conversion, and the digit representation of lnn_k_project.h in Python
integers.  Nothing here touches the device."""
import numpy as np

INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


def project_length(num_samples, hop):
    return 0 if hop == 0 else -(-num_samples // hop)


def frames_of(x, first, n, frame_len, hop, before):
    """x int (C, N_s) -> the frames [first, first + n) as int64 (C, n, frame_len): frame f holds samples f * hop - before + (0 .. N),
    zeros where that lies off the stream"""
    x = np.asarray(x, dtype=np.int64)
    C, Ns = x.shape
    lo = first * hop - before
    span = (n - 1) * hop + frame_len if n else 0
    img = np.zeros((C, span), dtype=np.int64)
    a, b = max(lo, 0), min(lo + span, Ns)
    if b > a:
        img[:, a - lo:b - lo] = x[:, a:b]
    idx = np.arange(n)[:, None] * hop + np.arange(frame_len)[None, :]
    return img[:, idx] if n else np.zeros((C, 0, frame_len), dtype=np.int64)


def projected_values(x, first, n, basis, hop, before=0, shift=0, clip_bits=0):
    """-> (y int64 (C, n, K), whether the clip changed an element).  The sums stay inside int64: 4096 products of at most 2^46"""
    basis = np.asarray(basis, dtype=np.int64)
    fr = frames_of(x, first, n, basis.shape[1], hop, before)
    acc = fr @ basis.T
    if shift:
        acc = (acc + (1 << (shift - 1))) >> shift
    B = clip_bits or 32
    y = np.clip(acc, -(1 << (B - 1)), (1 << (B - 1)) - 1)
    return y, bool((y != acc).any())


def expected_project(x, first, n, basis, hop, before=0, shift=0, clip_bits=0, f32=False, float_exp=0):
    """what the call stores: int32, or float32 (float)y * 2^-float_exp, as (C, n, K); and `saturated`"""
    y, sat = projected_values(x, first, n, basis, hop, before, shift, clip_bits)
    if not f32:
        return y.astype(np.int32), sat
    return (y.astype(np.int32).astype(np.float32) * np.float32(2.0 ** -float_exp)).astype(np.float32), sat


# ---- the digits of lnn_k_project.h, in Python integers ----
def s8(b):
    return b - 256 if b >= 128 else b


def basis_digits(v):
    """an int16 -> (lo', hi): v = 256 * hi + lo' + 128"""
    return (v & 255) - 128, v >> 8


def sample_planes(v):
    """the planes a sample needs: 2, 3 or 4"""
    m = v ^ (v >> 31)
    return 4 if m >= 1 << 23 else 3 if m >= 1 << 15 else 2


def sample_mask(P):
    return {2: 0x80, 3: 0x8080, 4: 0x808080}[P]


def sample_digits(v, P):
    """an int32 that fits 8 P bits -> its P digits: v = sum 256^b d_b + sample_mask(P)"""
    d = (v & 0xFFFFFFFF) ^ sample_mask(P)
    return [s8((d >> (8 * b)) & 255) for b in range(P)]


def dot_by_digits(row, xs, P):
    """sum row[n] * xs[n] the kernel's way: the plane products, the shared ones row and the row's sum of (v - 128)"""
    N, c = len(row), sample_mask(P)
    bd, xd = [basis_digits(v) for v in row], [sample_digits(v, P) for v in xs]
    planes = sum(sum(bd[n][a] * xd[n][b] for n in range(N)) << (8 * (a + b)) for a in range(2) for b in range(P))
    ones = sum(sum(xd[n][b] for n in range(N)) << (8 * b) for b in range(P))
    rsum = sum(v - 128 for v in row)
    return planes + c * rsum + 128 * (ones + N * c)
