"""objectkv_amd -- MI355X-native SST block encode/decode for ObjectKV's
segment format (drop-in under danthegoodman1/ObjectKV's sst package).

The hot path is libokv_sst.so (HIP kernels for gfx950 behind the C-ABI in
include/okv_sst.h).  Importing this package does not touch the GPU.
"""
from ._lib import build, lib  # noqa: F401
from .sst import (Decoded, Decoder, Encoded, Encoder, GpuSegmentWriter, Metadata,  # noqa: F401
                  OkvError, SegmentWriter, bytes_to_metadata, fetch_metadata, pack_rows,
                  synth_segment, xxh64)
from .bloom import DeviceBloom  # noqa: F401
from .get import DeviceIndex, get_rows  # noqa: F401
from .snap import DeviceSnapshot, snap_get_rows  # noqa: F401
from .range import gather_rows, seek_rows  # noqa: F401

__all__ = ["build", "lib", "Decoder", "Decoded", "DeviceBloom", "DeviceIndex", "get_rows",
           "DeviceSnapshot", "snap_get_rows", "seek_rows", "gather_rows",
           "Encoder", "Encoded",
           "GpuSegmentWriter",
           "Metadata", "OkvError", "SegmentWriter", "pack_rows",
           "bytes_to_metadata", "fetch_metadata", "synth_segment", "xxh64"]
