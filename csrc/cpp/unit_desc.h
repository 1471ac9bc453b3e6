// Column layout of the scan-unit descriptor tensor (int64 [nfiles*ncols,
// UD_NFIELDS], row = file * ncols + col): written by _cpp.read_unit_raw,
// read by _hip.decode_unit / _hip.scan_unit_uselast.
#pragma once

enum UnitDescField {
  UD_PRESENT = 0,
  UD_IS_STRING,
  UD_IS_LIST,  // element offsets in soffs, element payload at sbytes
  UD_IS_DICT,
  UD_ESIZE,  // physical element size in bytes (0 for strings)
  UD_NUM_VALUES,
  UD_NULL_COUNT,
  UD_VAL_OFF,
  UD_VAL_LEN,
  UD_VALIDITY_OFF,  // -1: no validity region
  UD_DICT_OFF,
  UD_DICT_LEN,
  UD_RUN_OFF,
  UD_RUN_CNT,
  UD_DENSE_N,
  UD_SOFF_OFF,
  UD_SBYTES_OFF,
  UD_SBYTES_LEN,
  // raw value pages decoded on the GPU (read_unit.h, `enc` table):
  // 0 = none, 1 = DELTA_BINARY_PACKED, 2 = BYTE_STREAM_SPLIT
  UD_ENC,
  UD_ENC_OFF,    // first row of the column in the enc table
  UD_ENC_CNT,    // its rows: page rows, then miniblock rows
  UD_ENC_PAGES,  // how many of them are page rows
  // string column whose bytes the GPU moves (read_unit.h, "GPU string
  // route"): 0 = host-assembled, UD_STR_PLAIN, UD_STR_DICT
  UD_STR,
  UD_NFIELDS
};

enum UnitStrKind { UD_STR_HOST = 0, UD_STR_PLAIN = 1, UD_STR_DICT = 2 };
