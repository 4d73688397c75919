"""The paths of csrc/primitives.hip (device-wide exclusive scan, stable LSD radix sort) that its newer callers rely on and that
tests/test_gpu_primitives_knn.py does not reach.  Numbers from primitives.hip: SCAN_TILE = 2048, SORT_TILE = 4096,
SORT_ROW_SCAN_MAX_BLOCKS = 640, SCAN_AUX_SLOTS = 32.

  1. the scan with more than 4096 blocks (the recursive branch) and with exactly 4096        test_scan_beyond_4096_blocks
  2. exclusive_scan_u32_sum: the aux total in 32 slots, one block, in == out == aux_in       test_scan_with_aux_total
  3. radix_sort_pairs_u64_dn: the count read on the device                                   test_sort_with_device_count
  4. sort_row_scan_kernel beyond one 512-column chunk, and the 640 / 641 boundary            test_sort_row_scan_band
  5. odd and even pass counts, partial last digits, u32 at 32 bits                           test_sort_u64_end_bits, test_sort_u32_end_bits
  6. the edges of a sort tile                                                                test_sort_tile_edges
  7. workspace sizes and one scratch for two primitives back to back on a stream             every test (see Window), test_shared_scratch_*

References are exact (np.cumsum in uint64 cast to uint32; np.argsort(keys & mask, kind="stable")) and every comparison is
assert_array_equal.  Every device buffer a primitive writes -- out, keys_out, vals_out, temp, the aux slots, and keys_in / vals_in, which
a sort of more than one pass uses as its second buffer -- is a Window: exactly the bytes the primitive may use, 256-byte aligned, inside
a larger allocation filled with 0xA5 whose 4096 bytes on either side are compared after every call.

Sort keys are random over all 64 (32) bits, so the bits at and above end_bit must be ignored for the order and carried along; values are
random words, not a permutation.  A second run per case uses skewed keys: 90 % of the pairs share the most significant digit below
end_bit, so ties dominate the last pass and only a stable sort gives the reference's order."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 4096
FILL = 0xA5
AUX_SLOTS = 32
TORCH_OF = {np.dtype(np.uint32): torch.int32, np.dtype(np.uint64): torch.int64}
SIGNED_OF = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}


def _lib():
    from adgs import _lib
    return _lib.lib()


def _stream(stream=None):
    return ctypes.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)


def on_device(array):
    """A device tensor with the bits of the numpy array (uint32 -> int32, uint64 -> int64)."""
    return torch.from_numpy(array.view(SIGNED_OF[array.dtype]).copy()).cuda()


class Window:
    """`nbytes` bytes a primitive may write, starting at a 256-byte boundary, with GUARD bytes of 0xA5 on either side."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self.raw = torch.full((self.nbytes + 2 * GUARD + 256,), FILL, dtype=torch.uint8, device="cuda")
        self.off = GUARD + (-(self.raw.data_ptr() + GUARD)) % 256
        self.ptr = self.raw.data_ptr() + self.off
        assert self.ptr % 256 == 0 and self.off + self.nbytes + GUARD <= self.raw.numel()

    @classmethod
    def of(cls, array):
        """A window that holds the numpy array (uint32 / uint64)."""
        w = cls(array.nbytes)
        w.view(array.dtype).copy_(on_device(array))
        return w

    def view(self, dtype):
        return self.raw[self.off:self.off + self.nbytes].view(TORCH_OF[np.dtype(dtype)])

    def numpy(self, dtype):
        return self.view(dtype).cpu().numpy().view(dtype)

    def check_guards(self, what):
        lo, hi = self.raw[self.off - GUARD:self.off], self.raw[self.off + self.nbytes:self.off + self.nbytes + GUARD]
        assert bool((lo == FILL).all()), "%s: bytes before the buffer were written" % what
        assert bool((hi == FILL).all()), "%s: bytes after the buffer were written" % what


def check_all_guards(windows, what):
    for name, w in windows.items():
        w.check_guards("%s, %s" % (what, name))


# ---------------------------------------------------------------------------------------------------------------- scan

def scan_reference(x):
    c = np.cumsum(x, dtype=np.uint64)
    return np.concatenate([np.zeros(1, np.uint64), c[:-1]]).astype(np.uint32)


@functools.lru_cache(maxsize=4)
def small_values(n):
    """n values in [0, 50) (nothing wraps below 85 M of them) with their exclusive scan."""
    x = np.random.default_rng(n).integers(0, 50, size=n, dtype=np.uint32)
    ref = scan_reference(x)
    x.setflags(write=False)
    ref.setflags(write=False)
    return x, ref


@pytest.mark.parametrize("n", [8_388_608, 8_388_609, 8_390_657])           # 4096 blocks (the last sums 4095 predecessors), 4097, 4098
def test_scan_beyond_4096_blocks(n):
    lib = _lib()
    x, ref = small_values(n)
    temp = Window(lib.adgs_test_scan_temp_bytes(n))
    src = on_device(x)
    out = Window(4 * n)
    assert lib.adgs_test_exclusive_scan_u32(src.data_ptr(), out.ptr, n, temp.ptr, _stream()) == 0
    np.testing.assert_array_equal(out.numpy(np.uint32), ref)
    check_all_guards(dict(out=out, temp=temp), "scan of %d" % n)
    np.testing.assert_array_equal(src.cpu().numpy().view(np.uint32), x)
    inplace = Window.of(x)
    assert lib.adgs_test_exclusive_scan_u32(inplace.ptr, inplace.ptr, n, temp.ptr, _stream()) == 0
    np.testing.assert_array_equal(inplace.numpy(np.uint32), ref)
    check_all_guards(dict(out=inplace, temp=temp), "scan of %d in place" % n)


def slot_sum(slots):
    return sum(int(v) for v in slots)


@pytest.mark.parametrize("form", ["no_aux", "separate_aux", "aliased"])
@pytest.mark.parametrize("n", [1, 2048, 2049, 70_001, 8_388_609])           # one block (the extra launch), its edge, two blocks, 35, the recursion
def test_scan_with_aux_total(n, form):
    lib = _lib()
    x, ref = small_values(n)
    rng = np.random.default_rng(7 * n + 1)
    temp = Window(lib.adgs_test_scan_temp_bytes(n))
    # the call ADDS to the slots: they start from other contents than zero except in the aliased form, which is how the callers run it
    start = np.zeros(AUX_SLOTS, np.uint64) if form == "aliased" else rng.integers(1, 1 << 40, size=AUX_SLOTS, dtype=np.uint64)
    slots = Window.of(start)
    what = "scan of %d, %s" % (n, form)
    if form == "aliased":                                                    # in == out == aux_in, as mesh, simplify and the TSDFs call it
        buf = Window.of(x)
        assert lib.adgs_test_exclusive_scan_u32_sum(buf.ptr, buf.ptr, n, temp.ptr, buf.ptr, slots.ptr, _stream()) == 0
        out, added = buf, int(x.sum(dtype=np.uint64))
    else:
        src = on_device(x)
        out = Window(4 * n)
        aux, added = None, 0
        if form == "separate_aux":                                           # values up to 2^31: from a few of them on the total needs 64 bits
            a = rng.integers(0, (1 << 31) + 1, size=n, dtype=np.uint32)
            a[0] = 1 << 31
            aux, added = on_device(a), int(a.sum(dtype=np.uint64))
            assert n < 4 or added > 1 << 32
        assert lib.adgs_test_exclusive_scan_u32_sum(src.data_ptr(), out.ptr, n, temp.ptr, None if aux is None else aux.data_ptr(), slots.ptr, _stream()) == 0
        np.testing.assert_array_equal(src.cpu().numpy().view(np.uint32), x)
        if aux is not None:
            np.testing.assert_array_equal(aux.cpu().numpy().view(np.uint32), a)
    np.testing.assert_array_equal(out.numpy(np.uint32), ref)
    after = slots.numpy(np.uint64)
    if form == "no_aux":
        np.testing.assert_array_equal(after, start)                          # untouched
    else:
        assert slot_sum(after) == slot_sum(start) + added, what
    check_all_guards(dict(out=out, temp=temp, slots=slots), what)


# ---------------------------------------------------------------------------------------------------------------- sort

def key_mask(dtype, end_bit):
    return np.dtype(dtype).type((1 << end_bit) - 1)


def skewed(keys, end_bit, seed):
    """90 % of the keys get one value in the most significant digit below end_bit (the last pass); every other bit stays as it is."""
    lo = 8 * ((end_bit - 1) // 8)
    digit = np.dtype(keys.dtype).type(((1 << (end_bit - lo)) - 1) << lo)
    rng = np.random.default_rng(seed)
    share = rng.random(len(keys)) < 0.9
    out = keys.copy()
    out[share] = (keys[share] & ~digit) | np.dtype(keys.dtype).type(int(rng.integers(0, 1 << (end_bit - lo))) << lo)
    return out


@functools.lru_cache(maxsize=4)
def sort_input(bits, n, seed):
    """n random keys over all `bits` bits and n random 32-bit values."""
    rng = np.random.default_rng((bits, n, seed))
    dtype = np.uint64 if bits == 64 else np.uint32
    keys = rng.integers(0, 1 << bits, size=n, dtype=dtype)
    vals = rng.integers(0, 1 << 32, size=n, dtype=np.uint32)
    keys.setflags(write=False)
    vals.setflags(write=False)
    return keys, vals


def sort_windows(keys, vals, temp=None):
    """The five buffers of a sort of these pairs; temp: exactly what the library reports for len(keys) pairs, unless one is handed in."""
    return dict(keys_in=Window.of(keys), vals_in=Window.of(vals), keys_out=Window(keys.nbytes), vals_out=Window(vals.nbytes),
                temp=temp or Window(_lib().adgs_test_sort_temp_bytes(len(keys))))


def launch_sort(w, dtype, n, end_bit, d_n=None, stream=None):
    lib = _lib()
    head = (w["keys_in"].ptr, w["keys_out"].ptr, w["vals_in"].ptr, w["vals_out"].ptr, n)
    if d_n is not None:
        return lib.adgs_test_sort_pairs_u64_dn(*head, d_n.data_ptr(), end_bit, w["temp"].ptr, _stream(stream))
    fn = lib.adgs_test_sort_pairs_u64 if np.dtype(dtype) == np.uint64 else lib.adgs_test_sort_pairs_u32
    return fn(*head, end_bit, w["temp"].ptr, _stream(stream))


def verify_sort(w, keys, vals, end_bit, what, m=None):
    """out[:m] is the stable sort of in[:m] on the key bits below end_bit (m: all); nothing outside the buffers was written."""
    m = len(keys) if m is None else m
    order = np.argsort(keys[:m] & key_mask(keys.dtype, end_bit), kind="stable")
    np.testing.assert_array_equal(w["keys_out"].numpy(keys.dtype)[:m], keys[:m][order], err_msg=what)
    np.testing.assert_array_equal(w["vals_out"].numpy(np.uint32)[:m], vals[:m][order], err_msg=what)
    check_all_guards(w, what)


def sort_and_verify(bits, n, end_bit, runs=("random", "skewed")):
    keys, vals = sort_input(bits, n, 0)
    for run in runs:
        k = skewed(keys, end_bit, n + end_bit) if run == "skewed" else keys
        w = sort_windows(k, vals)
        assert launch_sort(w, k.dtype, n, end_bit) == 0
        verify_sort(w, k, vals, end_bit, "u%d sort of %d pairs on %d bits, %s keys" % (bits, n, end_bit, run))


@pytest.mark.parametrize("n", [4095, 4096, 4097, 8193])
@pytest.mark.parametrize("bits,end_bit", [(32, 8), (64, 33)])
def test_sort_tile_edges(bits, end_bit, n):
    sort_and_verify(bits, n, end_bit)


# passes: 1, 1, 2, 2, 3, 3, 4, 5, 5, 6, 7, 8, 8 -- an odd count lands in keys_out, an even one is copied back; the last digit has 1 .. 8 bits
@pytest.mark.parametrize("end_bit", [1, 8, 9, 16, 17, 24, 25, 33, 40, 47, 56, 57, 63])
def test_sort_u64_end_bits(end_bit):
    sort_and_verify(64, 10_007, end_bit)


@pytest.mark.parametrize("end_bit", [1, 8, 9, 16, 17, 24, 25, 32])          # 32: the top bit counts (knn_points sorts negative floats' keys)
def test_sort_u32_end_bits(end_bit):
    sort_and_verify(32, 10_007, end_bit)


# 512, 513, 640 and 641 sort blocks: one chunk of the row scan, its carry into a second chunk, the last row scan, the first flat scan
@pytest.mark.parametrize("n", [2_097_152, 2_097_153, 2_621_440, 2_621_441])
@pytest.mark.parametrize("bits,end_bit", [(32, 16), (64, 8)])               # two passes (copied back); one pass (lands directly)
def test_sort_row_scan_band(bits, end_bit, n):
    sort_and_verify(bits, n, end_bit, runs=("skewed",))


POISON_VALUE = 0xDEADBEEF


def device_counts(n_cap):
    if n_cap >= 1_000_000:                                                   # two for the large capacity: blocks past the count, and the clamp
        return [n_cap // 2 + 1, n_cap + 1000]
    return sorted({0, 1, n_cap // 2 + 1, n_cap - 1, n_cap, n_cap + 1000})


DN_CASES = [(1, 64), (4096, 33), (10_000, 46), (10_000, 64), (2_700_000, 41)]


@pytest.mark.parametrize("n_cap,end_bit,count", [(c, e, d) for c, e in DN_CASES for d in device_counts(c)])
def test_sort_with_device_count(n_cap, end_bit, count):
    """The pairs at and beyond m = min(*d_n, n_cap) are poison: key 0, which would sort first if it were counted.  out[m:n_cap] is
    unspecified; the bytes beyond n_cap pairs and beyond sort_temp_bytes(n_cap) are not."""
    base_keys, base_vals = sort_input(64, n_cap, 1)
    m = min(count, n_cap)
    keys, vals = base_keys.copy(), base_vals.copy()
    keys[m:], vals[m:] = 0, POISON_VALUE
    w = sort_windows(keys, vals)
    d_n = torch.tensor([count], dtype=torch.int32, device="cuda")
    assert launch_sort(w, np.uint64, n_cap, end_bit, d_n=d_n) == 0
    verify_sort(w, keys, vals, end_bit, "sort of min(%d, %d) pairs on %d bits" % (count, n_cap, end_bit), m=m)
    assert int(d_n.item()) == count


# ---------------------------------------------------------------------------------------------------------------- one scratch, one stream

SHARED_N, SHARED_A = 9000, 700


def test_shared_scratch_two_sorts():
    """knn_points sorts its N points, then its A anchors, through one sort_temp on one stream, nothing in between."""
    lib = _lib()
    first, second = sort_input(32, SHARED_N, 2), sort_input(32, SHARED_A, 3)
    temp = Window(max(lib.adgs_test_sort_temp_bytes(SHARED_N), lib.adgs_test_sort_temp_bytes(SHARED_A)))
    assert temp.nbytes == lib.adgs_test_sort_temp_bytes(SHARED_N)
    w1, w2 = sort_windows(*first, temp=temp), sort_windows(*second, temp=temp)
    torch.cuda.synchronize()                                                 # the uploads ran on the default stream
    stream = torch.cuda.Stream()
    assert launch_sort(w1, np.uint32, SHARED_N, 32, stream=stream) == 0
    assert launch_sort(w2, np.uint32, SHARED_A, 32, stream=stream) == 0
    stream.synchronize()
    verify_sort(w1, *first, 32, "the first sort through a shared scratch")
    verify_sort(w2, *second, 32, "the second sort through a shared scratch")


def test_shared_scratch_sort_then_scan():
    """geometry sorts, then scans, through one scratch on one stream."""
    lib = _lib()
    keys, vals = sort_input(64, SHARED_N, 4)
    x, ref = small_values(SHARED_A)
    temp = Window(max(lib.adgs_test_sort_temp_bytes(SHARED_N), lib.adgs_test_scan_temp_bytes(SHARED_A)))
    w = sort_windows(keys, vals, temp=temp)
    src, out = on_device(x), Window(4 * SHARED_A)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    assert launch_sort(w, np.uint64, SHARED_N, 47, stream=stream) == 0
    assert lib.adgs_test_exclusive_scan_u32(src.data_ptr(), out.ptr, SHARED_A, temp.ptr, _stream(stream)) == 0
    stream.synchronize()
    verify_sort(w, keys, vals, 47, "the sort before a scan through a shared scratch")
    np.testing.assert_array_equal(out.numpy(np.uint32), ref)
    out.check_guards("the scan after a sort through a shared scratch")
