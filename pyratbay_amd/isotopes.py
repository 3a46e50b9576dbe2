"""Isotope ratios of sampled cross sections: the `isotope_ratios` block of the reference's
Line_Sample (pyratbay/opacity/line_sampling.py:142-238, 282-298, 374-456).  Every labelled opacity
file gets a table slot of its own; slots of one molecule share one atmospheric species, and each
slot's density is multiplied by its isotope ratio before the table is interpolated.  The ratios
that are not fillers are retrieval parameters `iso_<label>` (log10 of the ratio); a slot
`fill_A_B` takes 1 - (ratio of A + ratio of B).

Two forms of the same arithmetic:
  * the NumPy statements parse, assign, ratios_host and scale_host, which carry the specification;
  * IsotopeRatios.scale: temps[nw, L], dens[nw, L, nspec] and pars[nw, npars] -> the scaled device
    tensors, one launch of pb_iso_density (csrc/pb_isotopes.hip), nothing read back.

DEVIATIONS from the reference:
  * a filler that is itself a fill slot is refused (ValueError); the reference's result there
    depends on what the previous call left in the object;
  * at most MAX_ISO_FILLERS (7) fillers per fill slot -- below 8 terms np.sum is the sequential
    sum, so the device's sum has the host's bits -- and at most MAX_ISO_SLOTS (32) labelled slots;
  * a walker with any non-finite or negative ratio is REJECTED (bit REJECT_ISOTOPE): its
    temperatures and densities are 0 in every layer, WalkerAtmosphere's reject contract, which
    TableSpectrum.eval_bands turns into +inf band fluxes and the likelihood into -1e98.  The
    reference carries on with a negative opacity (NaN or a meaningless spectrum);
  * the ratios are stateless per walker; the reference keeps the last call's values in the object.
"""
import ctypes as C

import numpy as np

from ._capi import constant, struct
from .atmosphere import MAX_ISO_FILLERS, MAX_ISO_SLOTS, REJECT_ISOTOPE

KIND_CONST, KIND_FREE, KIND_FILL = (constant('PB_ISO_CONST'), constant('PB_ISO_FREE'),
                                    constant('PB_ISO_FILL'))
IsoModelStruct = struct('pb_iso_model')


def parse(block):
    """The `isotope_ratios` block -> [(key, 'iso_<label>', ratio)]: one line `key label ratio` per
    isotopologue; key, a substring of the opacity file's path; ratio, a float (log10 of the
    isotope ratio) or `fill_A_B...` (kept as the string it is)."""
    entries = []
    for line in block.strip().split('\n'):
        fields = line.split()
        if len(fields) != 3:
            raise ValueError(f"isotope_ratios: 'key label ratio' wanted, got '{line.strip()}'")
        key, label, ratio = fields
        if not ratio.startswith('fill_'):
            float(ratio)
        entries.append((key, 'iso_' + label, ratio))
    return entries


def assign(entries, cs_files, file_species):
    """The table slots of a list of opacity files: a key is a substring of the path (two keys in
    one path: ValueError); one slot per (species, label) in first-seen order, files of one slot
    are added; an unlabelled file takes its species' slot as without a block.
    -> (species[nspec], isotopes[nspec], slot of every file)."""
    slot_of, per_file = {}, []
    for path, sp in zip(cs_files, file_species):
        found = [label for key, label, _ in entries if key in path]
        if len(found) > 1:
            raise ValueError(f'Multiple isotope labels match {path!r}')
        slot = (str(sp), found[0] if found else '')
        per_file.append(slot_of.setdefault(slot, len(slot_of)))
    return [sp for sp, _ in slot_of], [label for _, label in slot_of], per_file


class IsotopeRatios:
    """IsotopeRatios(species, isotopes, entries): species[nspec] and isotopes[nspec] ('' or
    'iso_<label>') of the table's slots (assign), entries as parse() returns them.  Attributes
    under Line_Sample's names: species, isotopes, pnames (the free slots' labels, in slot order),
    pars (their log10 defaults), npars, iso_fill (per slot: None or the filler slots), iso_ratios
    (the defaults); and kind[nspec] (KIND_CONST for an unlabelled slot, KIND_FREE, KIND_FILL),
    par_column[nspec] (the column of pars a free slot reads, else -1), free_slots, labelled."""

    def __init__(self, species, isotopes, entries):
        self.species = np.array([str(s) for s in species])
        self.isotopes = [str(iso) for iso in isotopes]
        self.nspec = len(self.isotopes)
        if len(self.species) != self.nspec or self.nspec < 1:
            raise ValueError(f'species and isotopes: one entry per table slot, got '
                             f'{len(self.species)} and {self.nspec}')
        ratio_of = {label: ratio for _, label, ratio in entries}
        slot_of = {}
        for i, label in enumerate(self.isotopes):
            if label:
                slot_of.setdefault(label, i)
        self.labelled = [i for i, label in enumerate(self.isotopes) if label]
        if len(self.labelled) > MAX_ISO_SLOTS:
            raise ValueError(f'{len(self.labelled)} labelled isotope slots: at most '
                             f'{MAX_ISO_SLOTS}')
        missing = [self.isotopes[i] for i in self.labelled if self.isotopes[i] not in ratio_of]
        if missing:
            raise ValueError(f'{missing} are not labels of the isotope_ratios block')
        is_fill = np.array([bool(label) and ratio_of[label].startswith('fill_')
                            for label in self.isotopes])
        is_free = np.array([bool(label) for label in self.isotopes]) & ~is_fill
        self.kind = np.where(is_fill, KIND_FILL, np.where(is_free, KIND_FREE, KIND_CONST)
                             ).astype(np.int32)
        self.free_slots = [int(i) for i in np.flatnonzero(is_free)]
        self.par_column = np.full(self.nspec, -1, np.int32)
        self.par_column[self.free_slots] = np.arange(len(self.free_slots))
        self.pnames = [self.isotopes[i] for i in self.free_slots]
        self.pars = np.array([float(ratio_of[name]) for name in self.pnames], float)
        self.npars = len(self.pnames)
        self.iso_fill = [None] * self.nspec
        for i in np.flatnonzero(is_fill):
            parts = ratio_of[self.isotopes[i]][len('fill_'):].split('_')
            wanted = ['iso_' + part for part in parts]
            if any(name not in slot_of for name in wanted):
                raise ValueError('Invalid filler')
            if len(wanted) > MAX_ISO_FILLERS:
                raise ValueError(f"'{self.isotopes[i]}' has {len(wanted)} fillers: at most "
                                 f'{MAX_ISO_FILLERS}')
            self.iso_fill[i] = [slot_of[name] for name in wanted]
            nested = [self.isotopes[j] for j in self.iso_fill[i] if is_fill[j]]
            if nested:
                raise ValueError(f"'{self.isotopes[i]}': its filler '{nested[0]}' is a fill "
                                 'slot itself: name the free slots it stands for')
        # the defaults: Python's float power for the free slots (the reference's bits), the fill
        # slots by the host statement
        self.iso_ratios = np.ones(self.nspec)
        self.iso_ratios[self.free_slots] = [10.0**float(p) for p in self.pars]
        for i in np.flatnonzero(is_fill):
            total = 0.0
            for j in self.iso_fill[i]:
                total += self.iso_ratios[j]
            self.iso_ratios[i] = 1.0 - total
        self._struct = {}

    # ------------------------------------------------------------------ host statements
    def _pars_host(self, pars):
        pars = np.asarray(pars, dtype=np.float64)
        if pars.ndim != 2 or pars.shape[1] != self.npars:
            raise ValueError(f'iso_pars must have shape (nw, {self.npars}) ({self.pnames}), got '
                             f'{pars.shape}')
        return pars

    def ratios_host(self, pars):
        """pars[nw, npars] (log10) -> ratios[nw, nspec]: 1.0 for an unlabelled slot, 10.0**par for
        a free one, 1.0 - sum(fillers) for a fill slot, summed left to right in filler order."""
        pars = self._pars_host(pars)
        ratios = np.ones((pars.shape[0], self.nspec))
        with np.errstate(all='ignore'):
            if self.npars:
                ratios[:, self.free_slots] = 10.0**pars
            for i in self.labelled:
                if self.iso_fill[i] is not None:
                    total = ratios[:, self.iso_fill[i][0]].copy()
                    for j in self.iso_fill[i][1:]:
                        total = total + ratios[:, j]
                    ratios[:, i] = 1.0 - total
        return ratios

    def scale_host(self, temps, dens, pars=None):
        """temps[nw, L], dens[nw, L, nspec], pars[nw, npars] (None: the defaults) -> (temps, dens
        times the ratios, reject[nw]): a walker with a non-finite or negative ratio has
        reject = REJECT_ISOTOPE and zeros in both."""
        temps, dens = np.asarray(temps, float), np.asarray(dens, float)
        nw = temps.shape[0]
        if dens.shape != temps.shape + (self.nspec,):
            raise ValueError(f'dens must have shape {temps.shape + (self.nspec,)}, got '
                             f'{dens.shape}')
        ratios = np.tile(self.iso_ratios, (nw, 1)) if pars is None else self.ratios_host(pars)
        if ratios.shape[0] != nw:
            raise ValueError(f'iso_pars has {ratios.shape[0]} rows, temps {nw}')
        with np.errstate(invalid='ignore'):
            bad = np.any(~np.isfinite(ratios) | (ratios < 0.0), axis=1)
            out = dens * ratios[:, None, :]
        out[bad] = 0.0
        return (np.where(bad[:, None], 0.0, temps), out,
                np.where(bad, REJECT_ISOTOPE, 0).astype(np.int32))

    # ------------------------------------------------------------------ device form
    def model_struct(self, with_pars):
        """The pb_iso_model of this model; with_pars False: every free slot is a constant, its
        default as the host formed it."""
        if with_pars not in self._struct:
            st = IsoModelStruct()
            st.nspec, st.npars, st.nlabelled = self.nspec, self.npars, len(self.labelled)
            position = {slot: k for k, slot in enumerate(self.labelled)}
            for k, i in enumerate(self.labelled):
                st.slot[k], st.par[k], st.constant[k] = i, -1, 1.0
                if self.kind[i] == KIND_FILL:
                    st.kind[k], st.nfill[k] = KIND_FILL, len(self.iso_fill[i])
                    for m, j in enumerate(self.iso_fill[i]):
                        st.fill[k][m] = position[j]
                elif with_pars:
                    st.kind[k], st.par[k] = KIND_FREE, int(self.par_column[i])
                else:
                    st.kind[k], st.constant[k] = KIND_CONST, float(self.iso_ratios[i])
            self._struct[with_pars] = st
        return self._struct[with_pars]

    def check_pars(self, who, pars, nw):
        """pars: None or a float64 device tensor [nw, npars] (ValueError otherwise)."""
        import torch
        if pars is None:
            return
        if not isinstance(pars, torch.Tensor) or not pars.is_cuda or \
                pars.dtype != torch.float64 or tuple(pars.shape) != (nw, self.npars):
            raise ValueError(f'{who} must be a float64 device tensor of shape '
                             f'{(nw, self.npars)} ({self.pnames}), got {type(pars).__name__} '
                             f'{getattr(pars, "dtype", "")} {tuple(getattr(pars, "shape", ()))}')

    def scale(self, temps, dens, pars=None, want_ratios=False):
        """scale_host on the device (pb_iso_density, one launch): temps[nw, L], dens[nw, L, nspec],
        pars[nw, npars] or None (the defaults) -> (temps, dens, reject int32[nw], ratios[nw,
        nspec] or None), new tensors; the inputs are only read."""
        import torch
        from ._capi import call
        from ._device import _ptr, _stream
        nw, nlayers = temps.shape
        if tuple(dens.shape) != (nw, nlayers, self.nspec) or temps.dtype != torch.float64 or \
                dens.dtype != torch.float64 or not temps.is_cuda or not dens.is_cuda:
            raise ValueError(f'float64 device tensors temps[nw, L] and dens[nw, L, {self.nspec}] '
                             f'wanted, got {tuple(temps.shape)} and {tuple(dens.shape)}')
        self.check_pars('iso_pars', pars, nw)
        temps_in, dens_in = temps.contiguous(), dens.contiguous()
        pars_in = None if pars is None or self.npars == 0 else pars.contiguous()
        temps_out, dens_out = torch.empty_like(temps_in), torch.empty_like(dens_in)
        reject = torch.empty(nw, dtype=torch.int32, device=temps.device)
        ratios = torch.empty((nw, self.nspec), dtype=torch.float64, device=temps.device) \
            if want_ratios else None
        st = self.model_struct(pars_in is not None)
        call('pb_iso_density', _ptr(dens_out), _ptr(temps_out), _ptr(ratios), _ptr(reject),
             _ptr(dens_in), _ptr(temps_in), _ptr(pars_in), C.byref(st), nlayers, nw, _stream())
        return temps_out, dens_out, reject, ratios
