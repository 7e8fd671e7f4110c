/*
 * wfh5w.h -- C ABI of libwfh5w.so: raw-record reader / writer for the compound tables of the prediction writers
 * (reference WritePredictions.py -> src/datasets/PredictionWriter.py on src/datasets/HDF5IO.py H5Input / H5Output /
 * P2XTableWriter).
 *
 * A prediction file is a COPY of its input whose `EZ` / `phys` columns hold the model's output, so nothing here
 * converts anything: rows travel as the file's own compound records (reference: `self.table[a:b]` numpy records,
 * HDF5IO.py:55-79; `add_rows`, :95-97) between the file and a caller's HOST buffer, which may be page-locked for
 * the asynchronous copy to the device where csrc/predwrite.hip works on them.  include/wfh5.h stays the reader of the
 * training path (members converted to COO); this library has its own prefix and shares no state with it.
 *
 * Output tables are 1-D, extendible, gzip level 9 in chunks of 1024 rows (reference H5Output.create_table, :88-93).
 * The attribute / dataset setters exist for the fixture generator (tests/golden/make_prediction_fixtures.py): h5py is
 * not available to write test files with.
 *
 * Plain C types, caller-allocated buffers, no global state besides a thread-local error string.
 */
#ifndef WFH5W_H
#define WFH5W_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WFH5W_OK 0
#define WFH5W_EIO 1        /* file / object cannot be opened, read or written   */
#define WFH5W_EFORMAT 2    /* the table is not a 1-D dataset of a compound type */
#define WFH5W_EINVAL 3

/* element kinds of a member (little-endian, as the files are) */
#define WFH5W_I16 0
#define WFH5W_I32 1
#define WFH5W_I64 2
#define WFH5W_F32 3
#define WFH5W_F64 4
#define WFH5W_OTHER (-1)   /* reported for anything else; such a member still travels inside the raw records */

#define WFH5W_NAME_MAX 64

typedef struct wfh5w_member {
    char name[WFH5W_NAME_MAX];
    int64_t offset;        /* byte offset inside a record                        */
    int32_t kind;          /* WFH5W_I16 ...                                      */
    int32_t count;         /* elements per row (1 = scalar or array of one)      */
} wfh5w_member;

typedef struct wfh5w_in wfh5w_in;
typedef struct wfh5w_out wfh5w_out;

const char *wfh5w_last_error(void);

/* ---- input ---- */
int wfh5w_open_input(const char *path, const char *table, wfh5w_in **out);
void wfh5w_close_input(wfh5w_in *in);
int wfh5w_input_info(const wfh5w_in *in, int64_t *n_rows, int64_t *item_size, int32_t *n_members);
int wfh5w_input_member(const wfh5w_in *in, int32_t index, wfh5w_member *member);
/* rows [row0, row1) in the file's own compound layout; buf_bytes >= (row1 - row0) * item_size */
int wfh5w_read_records(wfh5w_in *in, int64_t row0, int64_t row1, void *buf, size_t buf_bytes);
/* one attribute of the open table: strings as their text (is_string = 1, n = length without the terminator),
 * numbers widened to float64 (is_string = 0, n = element count).  WFH5W_EIO when the table has no such attribute. */
int wfh5w_read_attr(const wfh5w_in *in, const char *name, void *buf, size_t buf_bytes, int32_t *is_string, int64_t *n);

/* ---- output ---- */
int wfh5w_create(const char *path, wfh5w_out **out);
int wfh5w_close(wfh5w_out *out);           /* closes the table and the file; the handle is gone whatever it returns */
/* a whole dataset of the input's FILE with its attributes (`Chanmap`: reference P2XTableWriter.copy_chanmap) */
int wfh5w_copy_dataset(wfh5w_out *out, const wfh5w_in *in, const char *name);
/* the output table (one per handle at a time: a second call closes the first table): the input table's own type and
 * name, or an explicit description */
int wfh5w_create_table_like(wfh5w_out *out, const wfh5w_in *in);
int wfh5w_create_table(wfh5w_out *out, const char *name, const wfh5w_member *members, int32_t n_members,
                       int64_t item_size);
int wfh5w_append(wfh5w_out *out, const void *records, int64_t n_rows);
int wfh5w_flush(wfh5w_out *out);
/* CLASS, FIELD_<n>_NAME, TITLE, VERSION, abstime, runtime, calgrp, nevents, rname, scalingfactor of the input table
 * onto the output table (reference P2XTableWriter.copy_p2x_attrs); an attribute the input lacks is skipped */
int wfh5w_copy_table_attrs(wfh5w_out *out, const wfh5w_in *in);
/* attributes of the output table, for files written from scratch: a fixed-length string (length + 1, as the
 * reference's H5T_C_S1 copies), float64 [1] */
int wfh5w_set_attr_string(wfh5w_out *out, const char *name, const char *value);
int wfh5w_set_attr_f64(wfh5w_out *out, const char *name, double value);

#ifdef __cplusplus
}
#endif
#endif /* WFH5W_H */
