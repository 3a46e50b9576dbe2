"""Line-by-line extinction on the device: the Voigt table, the line list, the partition-function
tables and the all-layer extinction plan (handles of the C ABI's objects)."""
import ctypes as C

import numpy as np
import torch

from ._capi import call, hptr, f64h, i32h
from ._device import _ptr, _stream, dev, require_gpu


# --------------------------------------------------------------------------
# Voigt table
# --------------------------------------------------------------------------
class VoigtTable:
    """Grid of Voigt profiles resident on the device (vprofile.grid, voigt.py:133-149)."""

    def __init__(self, handle, nlor, ndop, lorentz, doppler, osamp):
        self._h = handle
        self.nlor, self.ndop, self.osamp = nlor, ndop, osamp
        self.lorentz, self.doppler = lorentz, doppler
        size = np.zeros((nlor, ndop), np.int32)
        index = np.zeros((nlor, ndop), np.int32)
        n = C.c_int64(0)
        call('pb_voigt_meta', self._h, hptr(size), hptr(index), C.byref(n))
        self.size, self.index, self.nprofile = size, index, n.value

    @classmethod
    def build(cls, lorentz, doppler, size, ownstep, osamp, keep_flat=False):
        require_gpu()
        lorentz, doppler = f64h(lorentz), f64h(doppler)
        size = i32h(size)
        h = C.c_void_p()
        call('pb_voigt_create', C.byref(h), hptr(lorentz), len(lorentz), hptr(doppler),
             len(doppler), hptr(size), float(ownstep), int(osamp), int(keep_flat), _stream())
        return cls(h, len(lorentz), len(doppler), lorentz, doppler, int(osamp))

    @classmethod
    def from_flat(cls, profile, size, index, lorentz, doppler, osamp, keep_flat=False):
        require_gpu()
        profile, lorentz, doppler = f64h(profile), f64h(lorentz), f64h(doppler)
        size, index = i32h(size), i32h(index)
        h = C.c_void_p()
        call('pb_voigt_from_flat', C.byref(h), hptr(profile), profile.size, hptr(lorentz),
             len(lorentz), hptr(doppler), len(doppler), hptr(size), hptr(index), int(osamp),
             int(keep_flat), _stream())
        return cls(h, len(lorentz), len(doppler), lorentz, doppler, int(osamp))

    def flat(self, out=None):
        """The table in the reference's layout (what vprofile.grid fills), on the host."""
        if out is None:
            out = np.zeros(self.nprofile)
        assert out.dtype == np.float64 and out.flags.c_contiguous
        call('pb_voigt_flat_to_host', self._h, hptr(out), out.size)
        return out

    @property
    def device_bytes(self):
        return call('pb_voigt_device_bytes', self._h)

    def close(self):
        if self._h:
            call('pb_voigt_destroy', self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# --------------------------------------------------------------------------
# Line list
# --------------------------------------------------------------------------
class LineList:
    """Line transitions + the co-add groups of _extcoeff.c:243-262, on the device."""

    def __init__(self, lwn, elow, gf, lid, niso, own):
        require_gpu()
        lwn, elow, gf, lid, own = f64h(lwn), f64h(elow), f64h(gf), i32h(lid), f64h(own)
        self.nlines, self.niso = len(lwn), int(niso)
        self._h = C.c_void_p()
        call('pb_lines_create', C.byref(self._h), hptr(lwn), hptr(elow), hptr(gf), hptr(lid),
             len(lwn), int(niso), hptr(own), len(own), float(own[0]), float(own[1] - own[0]))
        st = (C.c_int64 * 3)()
        call('pb_lines_stats', self._h, C.byref(st))
        self.ninrange, self.ngroups, self.nadd = st[0], st[1], st[2]
        flag = C.c_int(0)
        call('pb_lines_grouped_on_device', self._h, C.byref(flag))
        self.grouped_on_device = bool(flag.value)

    def groups(self):
        """(first, count, iown)[ngroups] and iso_gstart[niso + 1] of the co-add groups."""
        first = np.zeros(self.ngroups, np.int32)
        count = np.zeros(self.ngroups, np.int32)
        iown = np.zeros(self.ngroups, np.int32)
        start = np.zeros(self.niso + 1, np.int64)
        call('pb_lines_groups', self._h, hptr(first), hptr(count), hptr(iown), hptr(start))
        return first, count, iown, start

    def close(self):
        if self._h:
            call('pb_lines_destroy', self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# --------------------------------------------------------------------------
# Partition functions Z_i(T)
# --------------------------------------------------------------------------
class PartitionTable:
    """The partition-function tables of a TLI file's databases on the device, evaluated at a
    temperature profile the way Line_By_Line does on every extinction call
    (pyratbay/pyrat/line_by_line.py:156-158: interp1d(db.temp, db.iso_pf[j], kind='slinear');
    :219-222: iso_pf[i] = iso_pf_interp[i](temperature)).  `databases`: the header dicts of
    pyratbay_amd.tli.read_tli (keys temperatures[ntemp], partition[niso, ntemp]); isotopes are
    numbered over the concatenated databases, as the line list's isotope index is."""

    def __init__(self, databases):
        require_gpu()
        self.tables = []
        self.niso = 0
        for db in databases:
            t = np.ascontiguousarray(db['temperatures'], float)
            pf = np.ascontiguousarray(np.atleast_2d(db['partition']), float)
            if t.size < 2 or pf.shape[1] != t.size or np.any(np.diff(t) <= 0):
                raise ValueError('partition-function table: temperatures must be strictly '
                                 'ascending (at least two) and match partition[niso, ntemp]')
            self.tables.append((dev(t), dev(pf), self.niso, pf.shape[0]))
            self.niso += pf.shape[0]
        self._nbad = torch.zeros(1, dtype=torch.int32, device='cuda')

    def evaluate(self, temp, out=None, check=True):
        """temp: device tensor of any shape [...] -> Z[niso, ...] (float64, device).  check=True
        waits for the kernel and raises ValueError for a temperature outside a table, like
        interp1d; check=False leaves NaN in those places and does not synchronise (a batch of
        walkers whose out-of-range members the caller rejects by their NaN spectra)."""
        temp = temp.contiguous()
        n = temp.numel()
        if out is None:
            out = torch.empty((self.niso,) + tuple(temp.shape), dtype=torch.float64,
                              device=temp.device)
        assert out.is_contiguous() and out.numel() == self.niso * n
        if check:
            self._nbad.zero_()
        for ttab, pf, first, niso in self.tables:
            call('pb_iso_partition', out.data_ptr() + 8 * first * n, n, 1, _ptr(temp), n,
                 _ptr(ttab), ttab.numel(), _ptr(pf), niso, _ptr(self._nbad) if check else None,
                 _stream())
        if check and int(self._nbad.item()) > 0:
            lo = max(float(t[0][0]) for t in self.tables)
            hi = min(float(t[0][-1]) for t in self.tables)
            raise ValueError('A value in the temperature profile lies outside the partition-'
                             f'function tables ({lo} - {hi} K)')
        return out


# --------------------------------------------------------------------------
# LBL extinction
# --------------------------------------------------------------------------
class LBL:
    """All-layer line-by-line extinction (the loop of extinction.py:170-213)."""

    def __init__(self, voigt, lines, wn, divisors, molrad, molmass, isoimol, isomass,
                 isoratio, isoiext, cutoff, ethresh, resolution=False, max_layers=256):
        self.voigt, self.lines = voigt, lines       # keep the handles alive
        wn = f64h(wn)
        self.nwave = len(wn)
        self.nmol, self.niso = len(molmass), len(isomass)
        isoiext = i32h(isoiext)
        self.nrows_sep = max(1, int(isoiext.max()) + 1)
        self.max_layers = max_layers
        self._h = C.c_void_p()
        args = [f64h(molrad), f64h(molmass), i32h(isoimol), f64h(isomass), f64h(isoratio)]
        div = i32h(divisors)
        call('pb_lbl_create', C.byref(self._h), voigt._h, lines._h, hptr(wn), len(wn),
             hptr(div), len(div), hptr(args[0]), hptr(args[1]), self.nmol,
             hptr(args[2]), hptr(args[3]), hptr(args[4]), hptr(isoiext), self.niso,
             float(cutoff), float(ethresh), int(bool(resolution)), int(max_layers))
        self.resolution = bool(resolution)
        self.gather_mode = 'auto'

    def set_isoiext(self, isoiext):
        isoiext = i32h(isoiext)
        call('pb_lbl_set_isoiext', self._h, hptr(isoiext))

    def set_ethresh(self, ethresh):
        call('pb_lbl_set_ethresh', self._h, float(ethresh))

    GATHER = {'auto': 0, 'global': 1, 'staged': 2, 'resident': 3, 'scatter': 4, 'rounds': 5,
              'dynamic': 6, 'wave': 7}

    def set_gather_mode(self, mode):
        """'auto' | 'global' | 'staged' | 'resident'; 'dynamic' (`resolution` plans: the layers'
        dynamic grids through constant-step sub-plans).  'scatter', 'rounds' and 'wave' are
        measured dead ends that only the experiments build of the library carries
        (libpbhip_exp.so, _capi.experiments()); the default library refuses them.  See pbhip.h:
        pb_lbl_set_gather_mode."""
        call('pb_lbl_set_gather_mode', self._h, self.GATHER[mode])
        self.gather_mode = mode

    def set_record_budget(self, nbytes):
        """Largest buffer of per-(layer, group) line records a call may allocate; beyond it the
        line list is walked in chunks (pb_lbl_set_record_budget)."""
        call('pb_lbl_set_record_budget', self._h, int(nbytes))

    @property
    def last_chunks(self):
        n = C.c_int(0)
        call('pb_lbl_last_chunks', self._h, C.byref(n))
        return n.value

    def set_concurrency(self, n):
        """The caller keeps n independent spectra in flight (pb_lbl_set_concurrency)."""
        call('pb_lbl_set_concurrency', self._h, int(n))

    @property
    def last_gather_kernel(self):
        m = C.c_int(0)
        call('pb_lbl_last_gather_mode', self._h, C.byref(m))
        base = {0: None, 1: 'k_ext_resample', 2: 'k_ext_staged', 3: 'k_ext_linterp',
                4: 'k_ext_scatter', 5: 'k_ext_rounds', 6: 'dynamic grids'}[m.value & 7]
        if m.value & 16:
            base = 'k_ext_wave+' + base
        return 'k_ext_resident+' + base if m.value & 8 else base

    def extinction(self, temp, dens, isoz, add=True, out=None, wbegin=0, wcount=None):
        """temp[L], dens[L,nmol], isoz[niso,L] device tensors -> ec[L,rows,wcount]."""
        nlayers = temp.shape[0]
        if wcount is None:
            wcount = self.nwave - wbegin
        rows = 1 if add else self.nrows_sep
        if out is None:
            alloc = torch.zeros if self.resolution else torch.empty
            out = alloc((nlayers, rows, wcount), dtype=torch.float64, device=temp.device)
        assert out.shape == (nlayers, rows, wcount) and out.is_contiguous()
        assert dens.shape == (nlayers, self.nmol) and isoz.shape == (self.niso, nlayers)
        call('pb_lbl_extinction', self._h, _ptr(out), int(wbegin), int(wcount), _ptr(temp),
             _ptr(dens), _ptr(isoz), isoz.stride(0), isoz.stride(1), nlayers, int(bool(add)),
             _stream())
        return out

    def extinction_begin(self, temp, dens, isoz, add=True, out=None, wbegin=0, wcount=None):
        """First half of extinction() for a wavenumber shard of a multi-GPU run: layer state +
        the records of the groups within reach of the shard, per-row maxima over those groups
        only.  All-reduce (MAX) kmax_tensor() over the ranks, then call extinction_end()."""
        nlayers = temp.shape[0]
        if wcount is None:
            wcount = self.nwave - wbegin
        rows = 1 if add else self.nrows_sep
        if out is None:
            alloc = torch.zeros if self.resolution else torch.empty
            out = alloc((nlayers, rows, wcount), dtype=torch.float64, device=temp.device)
        assert out.shape == (nlayers, rows, wcount) and out.is_contiguous()
        assert dens.shape == (nlayers, self.nmol) and isoz.shape == (self.niso, nlayers)
        call('pb_lbl_extinction_begin', self._h, _ptr(out), int(wbegin), int(wcount), _ptr(temp),
             _ptr(dens), _ptr(isoz), isoz.stride(0), isoz.stride(1), nlayers, int(bool(add)),
             _stream())
        return out

    def kmax_tensor(self):
        """The per-(layer, row) maxima of the plan as an int64 device tensor that ALIASES the
        library's buffer (bit patterns of non-negative doubles: integer MAX = double max)."""
        if getattr(self, '_kmax', None) is None:
            ptr, n = C.c_void_p(), C.c_int64(0)
            call('pb_lbl_kmax_buffer', self._h, C.byref(ptr), C.byref(n))

            class _Alias:
                __cuda_array_interface__ = {'shape': (n.value,), 'typestr': '<i8',
                                            'data': (ptr.value, False), 'version': 2}
            self._kmax = torch.as_tensor(_Alias(), device='cuda')
        return self._kmax

    def extinction_end(self):
        call('pb_lbl_extinction_end', self._h, _stream())

    def timing_begin(self, max_launches):
        call('pb_lbl_timing_begin', self._h, int(max_launches))

    def timing_end(self):
        """(summed gather-kernel milliseconds, launches) since timing_begin()."""
        ms, n = C.c_double(0), C.c_int(0)
        call('pb_lbl_timing_end', self._h, C.byref(ms), C.byref(n))
        return ms.value, n.value

    def last_work(self):
        """{fma_lanes_useful, fma_lanes_issued, live_records} of the last call, counted on the
        device (pb_lbl_last_work); None when that launch kept no packed records."""
        w = (C.c_int64 * 3)()
        call('pb_lbl_last_work', self._h, C.byref(w), _stream())
        if w[0] < 0:
            return None
        return dict(fma_lanes_useful=int(w[0]), fma_lanes_issued=int(w[1]),
                    live_records=int(w[2]))

    def last_table_samples(self):
        """Distinct Voigt-table samples the live records of the last call select (None when not
        counted): pb_lbl_last_table_samples."""
        n = C.c_int64(-1)
        call('pb_lbl_last_table_samples', self._h, C.byref(n), _stream())
        return None if n.value < 0 else int(n.value)

    def last_state(self, nlayers, rows):
        ofactor = np.zeros(nlayers, np.int32)
        kmax = np.zeros((nlayers, rows))
        call('pb_lbl_last_state', self._h, hptr(ofactor), hptr(kmax), nlayers, rows,
             _stream())
        return ofactor, kmax

    def last_layer_kinds(self, nlayers):
        """(resident[L] 0/1, block[L] doubles) of the last call: pb_lbl_last_layer_kinds."""
        resident = np.zeros(nlayers, np.int32)
        block = np.zeros(nlayers, np.int32)
        call('pb_lbl_last_layer_kinds', self._h, hptr(resident), hptr(block), nlayers, _stream())
        return resident, block

    def last_rows_per_step(self, nlayers, niso):
        """rows[L, niso]: segments per barrier step of the staged gather in every (layer,
        isotope) of the last call (pb_lbl_last_rows_per_step)."""
        rows = np.zeros((nlayers, niso), np.int32)
        call('pb_lbl_last_rows_per_step', self._h, hptr(rows), nlayers, niso, _stream())
        return rows

    def last_wave_layers(self, nlayers):
        """wave[L] 0/1: the layers of the last call the wave-autonomous kernel computed."""
        wave = np.zeros(nlayers, np.int32)
        call('pb_lbl_last_wave_layers', self._h, hptr(wave), nlayers, _stream())
        return wave

    def set_dyn_predict(self, on=True):
        """`resolution` plans, gather mode 'dynamic': plan every call from the last read-back of
        the layers' oversampling factors instead of synchronising the stream (pbhip.h:
        pb_lbl_set_dyn_predict); needed to capture such a call into a HIP graph."""
        call('pb_lbl_set_dyn_predict', self._h, int(bool(on)))

    def dyn_stats(self):
        """`resolution` plans, gather mode 'dynamic': (calls planned from the last read-back of the
        layers' factors -- no stream synchronisation --, synchronous calls, read-backs that
        contradicted the prediction their call was planned with)."""
        st = np.zeros(3, np.int64)
        call('pb_lbl_dyn_stats', self._h, hptr(st))
        return tuple(int(v) for v in st)

    def close(self):
        if self._h:
            call('pb_lbl_destroy', self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
