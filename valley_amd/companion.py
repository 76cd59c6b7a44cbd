"""The loader every companion library shares (libvalley_hip_<name>.so, include/valley_hip_<name>.h).

A companion carries its own ABI version and the entry points vly_<name>_abi_version / vly_<name>_last_error; it is mapped
on first use, never on import.  Missing, incomplete or of another ABI version, it fails loudly: no companion has a
non-HIP path.  A binding module lib_<name>.py holds the signatures and one Companion, whose methods it re-exports."""
from __future__ import annotations

import ctypes
import os
import threading

from .lib import ValleyHipError, bind


class Companion:
    def __init__(self, name: str, sigs: dict, abi_version: int, default_path: str, no_fallback: str, label: str | None = None):
        self.name, self.sigs, self.abi_version, self.default_path = name, sigs, abi_version, default_path
        self.no_fallback = no_fallback              # the feature's sentence of the missing-library error
        self.label = label or name                  # what the ABI-mismatch error calls the library
        self._lib = None
        self._lock = threading.Lock()

    def lib_path(self) -> str:
        return os.environ.get(f"VALLEY_HIP_{self.name.upper()}_LIB", self.default_path)

    def loaded(self) -> bool:
        return self._lib is not None

    def reset(self) -> None:
        """Forget the handle: the next load() resolves lib_path() again (the tests of a missing library)."""
        with self._lock:
            self._lib = None

    def load(self):
        """Load (once) and type the library.  Raises if it is absent, incomplete or of another ABI version."""
        lib = self._lib
        if lib is not None:
            return lib
        with self._lock:
            if self._lib is not None:
                return self._lib
            path = self.lib_path()
            if not os.path.exists(path):
                raise ValleyHipError(f"{path} not found: build it with `python -m valley_amd.build` (hipcc --offload-arch=gfx950). "
                                     f"{self.no_fallback}")
            lib = ctypes.CDLL(path)
            bind(lib, path, self.sigs)
            got = getattr(lib, f"vly_{self.name}_abi_version")()
            if got != self.abi_version:
                raise ValleyHipError(f"{self.label} ABI mismatch: library {got} vs binding {self.abi_version}")
            self._lib = lib
            return lib

    def check(self, rc: int, what: str):
        if rc != 0:
            msg = getattr(self.load(), f"vly_{self.name}_last_error")().decode(errors="replace")
            raise ValleyHipError(f"{what} failed (rc={rc}): {msg}")
