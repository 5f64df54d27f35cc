"""The device handle of a keyed consumer of the ``--sv`` scan (csrc/tdt_keystore.h: a store of (K1, K2) keys in HBM, one push per batch,
one finish per job), written once for ``IndelCounter`` / ``SnvCounter`` / ``ClipCounter``.  A subclass names its C prefix and its ``SN``
size, creates the handle in its constructor (:meth:`_create`) and adds what is its own."""
import ctypes

import numpy

from . import _native, bamio


class KeyedCounter:
    PREFIX = None               # "tdt_indel": the entries are PREFIX_create, PREFIX_push, ...
    SIZE = 0                    # the SN rows of finish()
    DEFAULT_SUPPORT = 1
    ROW_DTYPES = (numpy.uint64, numpy.uint64, numpy.uint32, numpy.uint32)      # K1, K2 with bit 0 clear, SUPPORT, REV
    N_TIMES = 4
    depth = None                # a tiddit_pileup.PileupDepth the scan filled beside this counter (TIDDIT_SMALL_VCF): the caller's to finish and close

    def _create(self, ctx, *args):
        """``PREFIX_create(ctx, *args, &handle)``"""
        self.ctx = ctx or _native.default_context()
        assert self._c("sn_size")() == self.SIZE
        h = ctypes.c_void_p()
        _native.check(self._c("create")(self.ctx.handle, *args, ctypes.byref(h)))
        self.handle = h
        self._n_rows = 0
        self.reference = None                                   # what a subclass keeps alive until close()

    def _c(self, entry):
        return getattr(self.ctx.lib, self.PREFIX + "_" + entry)

    def _out(self, entry, n, dtype):
        out = numpy.zeros(n, dtype=dtype)
        _native.check(self._c(entry)(self.handle, _native.ptr(out)))
        return out

    def push_device_batch(self, b):
        """one DeviceBatch: enqueued on the reader's stream; nothing is waited for unless the reserve must ask or grow (call before the
        batch's buffers are handed on)"""
        _native.check(self._c("push_device")(self.handle, b.pointer_table(), len(b), b._raw_len))

    def push_host_batch(self, b):
        """one host-decoded batch (or any object with its columns): uploaded, then the same kernel"""
        cols, raw = bamio.host_columns(b, ("flag", "tid", "pos", "mapq", "rec_off"))            # (the arguments of PREFIX_push, in order)
        _native.check(self._c("push")(self.handle, *[_native.ptr(c) for c in cols], len(cols[0]), _native.ptr(raw), len(raw)))

    def keys(self):
        """-> (K1 uint64[], K2 uint64[]): the store as it lies in HBM (its order is not the file's)"""
        n = ctypes.c_size_t(0)
        _native.check(self._c("keys")(self.handle, None, None, ctypes.byref(n)))
        k1, k2 = numpy.zeros(n.value, dtype=numpy.uint64), numpy.zeros(n.value, dtype=numpy.uint64)
        if n.value:
            _native.check(self._c("keys")(self.handle, _native.ptr(k1), _native.ptr(k2), ctypes.byref(n)))
        return k1, k2

    def finish(self, min_support=None):
        """-> uint64[SIZE]: the push counters and, from one sort of the store, the sets (the store is left as it was)"""
        out = numpy.zeros(self.SIZE, dtype=numpy.uint64)
        n = ctypes.c_size_t(0)
        s = self.DEFAULT_SUPPORT if min_support is None else min_support
        _native.check(self._c("finish")(self.handle, int(s), _native.ptr(out), ctypes.byref(n)))
        self._n_rows = n.value
        return out

    def rows(self):
        """-> the columns of the last finish's rows (``ROW_DTYPES``), ascending by key"""
        n = ctypes.c_size_t(self._n_rows)
        cols = [numpy.zeros(n.value, dtype=dt) for dt in self.ROW_DTYPES]
        if n.value:
            _native.check(self._c("rows")(self.handle, *[_native.ptr(c) for c in cols], ctypes.byref(n)))
        return tuple(cols)

    def timing(self):
        """ms of the last finish: [sort by K2, gather, sort by K1, run lengths + rows]"""
        return self._out("timing", self.N_TIMES, numpy.float64)

    def reserve_stats(self):
        """-> (how often the reserve asked the device for the real count, how often the store grew, its capacity now)"""
        return tuple(int(v) for v in self._out("reserve_stats", 3, numpy.uint64))

    def reset(self):
        _native.check(self._c("reset")(self.handle))
        self._n_rows = 0

    def close(self):
        if getattr(self, "handle", None):
            self._c("destroy")(self.handle)
            self.handle = None
            self.reference = None                               # (only now: the handle's last kernel is done)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
