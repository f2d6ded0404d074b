"""MI355X-native witness engine for Blobstream X `header_range` (host side; the kernels live in csrc/, the C ABI in
include/bsx.h)."""
