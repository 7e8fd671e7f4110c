// h5writer.cpp -- libwfh5w.so (include/wfh5w.h): compound tables as raw records, in and out, over libhdf5.
// The reference moves the same records as numpy structured arrays through h5py (src/datasets/HDF5IO.py); here they go
// between the file and a caller's (page-locked) buffer untouched, in the FILE's compound type, so that the device can
// patch the prediction columns in place (csrc/predwrite.hip) and every other byte of a row is written back as read.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include <hdf5.h>

#include "../../include/wfh5w.h"

namespace {

thread_local char g_error[512] = "";

int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
    return code;
}

void quiet() { H5Eset_auto2(H5E_DEFAULT, nullptr, nullptr); }

const hsize_t CHUNK_ROWS = 1024;      // reference H5Output.create_table: chunks=(1024,), gzip 9

int kind_of(hid_t t) {
    const H5T_class_t c = H5Tget_class(t);
    const size_t s = H5Tget_size(t);
    if (c == H5T_INTEGER && H5Tget_sign(t) == H5T_SGN_2) return s == 2 ? WFH5W_I16 : s == 4 ? WFH5W_I32 : s == 8 ? WFH5W_I64 : WFH5W_OTHER;
    if (c == H5T_FLOAT) return s == 4 ? WFH5W_F32 : s == 8 ? WFH5W_F64 : WFH5W_OTHER;
    return WFH5W_OTHER;
}

hid_t type_of(int kind) {
    switch (kind) {
        case WFH5W_I16: return H5T_STD_I16LE;
        case WFH5W_I32: return H5T_STD_I32LE;
        case WFH5W_I64: return H5T_STD_I64LE;
        case WFH5W_F32: return H5T_IEEE_F32LE;
        case WFH5W_F64: return H5T_IEEE_F64LE;
    }
    return -1;
}

size_t size_of(int kind) { return kind == WFH5W_I16 ? 2 : (kind == WFH5W_I32 || kind == WFH5W_F32) ? 4 : 8; }

}  // namespace

struct wfh5w_in {
    hid_t file = -1, dset = -1, type = -1;
    std::string table;
    int64_t n_rows = 0, item_size = 0;
    std::vector<wfh5w_member> members;
};

struct wfh5w_out {
    hid_t file = -1, dset = -1, type = -1;
    int64_t rows = 0, item_size = 0;
};

extern "C" const char *wfh5w_last_error(void) { return g_error; }

extern "C" void wfh5w_close_input(wfh5w_in *in) {
    if (!in) return;
    if (in->type >= 0) H5Tclose(in->type);
    if (in->dset >= 0) H5Dclose(in->dset);
    if (in->file >= 0) H5Fclose(in->file);
    delete in;
}

extern "C" int wfh5w_open_input(const char *path, const char *table, wfh5w_in **out) {
    if (!path || !table || !out) return fail(WFH5W_EINVAL, "NULL argument");
    *out = nullptr;
    quiet();
    wfh5w_in *in = new wfh5w_in;
    in->table = table;
    int rc = WFH5W_OK;
    hid_t space = -1;
    do {
        in->file = H5Fopen(path, H5F_ACC_RDONLY, H5P_DEFAULT);
        if (in->file < 0) { rc = fail(WFH5W_EIO, "cannot open %s", path); break; }
        if (H5Lexists(in->file, table, H5P_DEFAULT) <= 0) { rc = fail(WFH5W_EIO, "%s has no table %s", path, table); break; }
        H5O_info_t oi;
        if (H5Oget_info_by_name2(in->file, table, &oi, H5O_INFO_BASIC, H5P_DEFAULT) < 0 || oi.type != H5O_TYPE_DATASET) {
            rc = fail(WFH5W_EFORMAT, "%s:%s is not a dataset", path, table);
            break;
        }
        in->dset = H5Dopen2(in->file, table, H5P_DEFAULT);
        if (in->dset < 0) { rc = fail(WFH5W_EIO, "cannot open %s:%s", path, table); break; }
        in->type = H5Dget_type(in->dset);
        if (in->type < 0 || H5Tget_class(in->type) != H5T_COMPOUND) {
            rc = fail(WFH5W_EFORMAT, "%s:%s is not of a compound type", path, table);
            break;
        }
        space = H5Dget_space(in->dset);
        hsize_t dims[1] = {0};
        if (space < 0 || H5Sget_simple_extent_ndims(space) != 1 || H5Sget_simple_extent_dims(space, dims, nullptr) != 1) {
            rc = fail(WFH5W_EFORMAT, "%s:%s is not one-dimensional", path, table);
            break;
        }
        in->n_rows = (int64_t)dims[0];
        in->item_size = (int64_t)H5Tget_size(in->type);
        const int nm = H5Tget_nmembers(in->type);
        if (nm <= 0 || in->item_size <= 0) { rc = fail(WFH5W_EFORMAT, "%s:%s has an empty compound type", path, table); break; }
        for (int i = 0; i < nm && rc == WFH5W_OK; ++i) {
            wfh5w_member m;
            memset(&m, 0, sizeof(m));
            char *name = H5Tget_member_name(in->type, (unsigned)i);
            hid_t mt = H5Tget_member_type(in->type, (unsigned)i);
            if (!name || mt < 0) {
                rc = fail(WFH5W_EFORMAT, "%s:%s member %d cannot be described", path, table, i);
            } else {
                snprintf(m.name, sizeof(m.name), "%s", name);
                m.offset = (int64_t)H5Tget_member_offset(in->type, (unsigned)i);
                m.count = 1;
                if (H5Tget_class(mt) == H5T_ARRAY) {
                    hsize_t ad[H5S_MAX_RANK];
                    const int nd = H5Tget_array_dims2(mt, ad);
                    int64_t c = 1;
                    for (int d = 0; d < nd; ++d) c *= (int64_t)ad[d];
                    hid_t base = H5Tget_super(mt);
                    m.kind = base >= 0 ? kind_of(base) : WFH5W_OTHER;
                    if (base >= 0) H5Tclose(base);
                    m.count = (int32_t)c;
                } else {
                    m.kind = kind_of(mt);
                }
                // a damaged header must not describe a member outside its record
                const int64_t bytes = m.kind == WFH5W_OTHER ? (int64_t)H5Tget_size(mt) : (int64_t)size_of(m.kind) * m.count;
                if (m.offset < 0 || m.count <= 0 || bytes <= 0 || m.offset + bytes > in->item_size)
                    rc = fail(WFH5W_EFORMAT, "%s:%s member %s lies outside its record", path, table, m.name);
                in->members.push_back(m);
            }
            if (name) H5free_memory(name);
            if (mt >= 0) H5Tclose(mt);
        }
    } while (0);
    if (space >= 0) H5Sclose(space);
    if (rc != WFH5W_OK) {
        wfh5w_close_input(in);
        return rc;
    }
    *out = in;
    return WFH5W_OK;
}

extern "C" int wfh5w_input_info(const wfh5w_in *in, int64_t *n_rows, int64_t *item_size, int32_t *n_members) {
    if (!in) return fail(WFH5W_EINVAL, "NULL handle");
    if (n_rows) *n_rows = in->n_rows;
    if (item_size) *item_size = in->item_size;
    if (n_members) *n_members = (int32_t)in->members.size();
    return WFH5W_OK;
}

extern "C" int wfh5w_input_member(const wfh5w_in *in, int32_t index, wfh5w_member *member) {
    if (!in || !member) return fail(WFH5W_EINVAL, "NULL argument");
    if (index < 0 || (size_t)index >= in->members.size())
        return fail(WFH5W_EINVAL, "member %d of %zu", index, in->members.size());
    *member = in->members[(size_t)index];
    return WFH5W_OK;
}

extern "C" int wfh5w_read_records(wfh5w_in *in, int64_t row0, int64_t row1, void *buf, size_t buf_bytes) {
    if (!in) return fail(WFH5W_EINVAL, "NULL handle");
    if (row0 < 0 || row1 < row0 || row1 > in->n_rows)
        return fail(WFH5W_EINVAL, "rows [%lld, %lld) of a table of %lld", (long long)row0, (long long)row1, (long long)in->n_rows);
    const int64_t n = row1 - row0;
    if (n == 0) return WFH5W_OK;
    if (!buf || (uint64_t)buf_bytes / (uint64_t)in->item_size < (uint64_t)n)
        return fail(WFH5W_EINVAL, "buffer of %zu bytes for %lld records of %lld bytes", buf_bytes, (long long)n, (long long)in->item_size);
    quiet();
    hid_t fspace = H5Dget_space(in->dset);
    const hsize_t start[1] = {(hsize_t)row0}, count[1] = {(hsize_t)n};
    hid_t mspace = H5Screate_simple(1, count, nullptr);
    int rc = WFH5W_OK;
    if (fspace < 0 || mspace < 0 || H5Sselect_hyperslab(fspace, H5S_SELECT_SET, start, nullptr, count, nullptr) < 0 ||
        H5Dread(in->dset, in->type, mspace, fspace, H5P_DEFAULT, buf) < 0)
        rc = fail(WFH5W_EIO, "short read of rows [%lld, %lld) of %s", (long long)row0, (long long)row1, in->table.c_str());
    if (mspace >= 0) H5Sclose(mspace);
    if (fspace >= 0) H5Sclose(fspace);
    return rc;
}

extern "C" int wfh5w_read_attr(const wfh5w_in *in, const char *name, void *buf, size_t buf_bytes, int32_t *is_string,
                               int64_t *n) {
    if (!in || !name || !buf || !is_string || !n) return fail(WFH5W_EINVAL, "NULL argument");
    quiet();
    if (H5Aexists(in->dset, name) <= 0) return fail(WFH5W_EIO, "%s has no attribute %s", in->table.c_str(), name);
    hid_t a = H5Aopen(in->dset, name, H5P_DEFAULT);
    if (a < 0) return fail(WFH5W_EIO, "cannot open attribute %s", name);
    hid_t t = H5Aget_type(a), s = H5Aget_space(a);
    int rc = WFH5W_OK;
    const hssize_t np = s >= 0 ? H5Sget_simple_extent_npoints(s) : -1;
    if (t < 0 || np < 0) {
        rc = fail(WFH5W_EIO, "attribute %s cannot be described", name);
    } else if (H5Tget_class(t) == H5T_STRING) {
        *is_string = 1;
        if (np != 1) {
            rc = fail(WFH5W_EFORMAT, "attribute %s is an array of strings", name);
        } else if (H5Tis_variable_str(t) > 0) {
            char *p = nullptr;
            hid_t mt = H5Tcopy(H5T_C_S1);
            H5Tset_size(mt, H5T_VARIABLE);
            H5Tset_cset(mt, H5Tget_cset(t));
            if (H5Aread(a, mt, &p) < 0 || !p) {
                rc = fail(WFH5W_EIO, "cannot read attribute %s", name);
            } else {
                const size_t len = strlen(p);
                if (len + 1 > buf_bytes) rc = fail(WFH5W_EINVAL, "attribute %s needs %zu bytes", name, len + 1);
                else { memcpy(buf, p, len + 1); *n = (int64_t)len; }
                H5free_memory(p);
            }
            H5Tclose(mt);
        } else {
            const size_t sz = H5Tget_size(t);
            std::vector<char> tmp(sz + 1, 0);
            if (H5Aread(a, t, tmp.data()) < 0) {
                rc = fail(WFH5W_EIO, "cannot read attribute %s", name);
            } else {
                const size_t len = strnlen(tmp.data(), sz);
                if (len + 1 > buf_bytes) rc = fail(WFH5W_EINVAL, "attribute %s needs %zu bytes", name, len + 1);
                else { memcpy(buf, tmp.data(), len); ((char *)buf)[len] = 0; *n = (int64_t)len; }
            }
        }
    } else if (H5Tget_class(t) == H5T_INTEGER || H5Tget_class(t) == H5T_FLOAT) {
        *is_string = 0;
        if ((uint64_t)np > buf_bytes / sizeof(double)) rc = fail(WFH5W_EINVAL, "attribute %s needs %lld doubles", name, (long long)np);
        else if (np > 0 && H5Aread(a, H5T_NATIVE_DOUBLE, buf) < 0) rc = fail(WFH5W_EIO, "cannot read attribute %s", name);
        else *n = (int64_t)np;
    } else {
        rc = fail(WFH5W_EFORMAT, "attribute %s is neither text nor numbers", name);
    }
    if (s >= 0) H5Sclose(s);
    if (t >= 0) H5Tclose(t);
    H5Aclose(a);
    return rc;
}

// ---------------------------------------------------------------------------------------------------------------------

static void close_table(wfh5w_out *o) {
    if (o->type >= 0) H5Tclose(o->type);
    if (o->dset >= 0) H5Dclose(o->dset);
    o->type = o->dset = -1;
    o->rows = o->item_size = 0;
}

extern "C" int wfh5w_create(const char *path, wfh5w_out **out) {
    if (!path || !out) return fail(WFH5W_EINVAL, "NULL argument");
    *out = nullptr;
    quiet();
    hid_t f = H5Fcreate(path, H5F_ACC_TRUNC, H5P_DEFAULT, H5P_DEFAULT);
    if (f < 0) return fail(WFH5W_EIO, "cannot create %s", path);
    wfh5w_out *o = new wfh5w_out;
    o->file = f;
    *out = o;
    return WFH5W_OK;
}

extern "C" int wfh5w_close(wfh5w_out *o) {
    if (!o) return fail(WFH5W_EINVAL, "NULL handle");
    quiet();
    close_table(o);
    const herr_t e = H5Fclose(o->file);
    delete o;
    return e < 0 ? fail(WFH5W_EIO, "closing the output file failed") : WFH5W_OK;
}

extern "C" int wfh5w_copy_dataset(wfh5w_out *o, const wfh5w_in *in, const char *name) {
    if (!o || !in || !name) return fail(WFH5W_EINVAL, "NULL argument");
    quiet();
    if (H5Lexists(in->file, name, H5P_DEFAULT) <= 0) return fail(WFH5W_EIO, "the input has no dataset %s", name);
    if (H5Ocopy(in->file, name, o->file, name, H5P_DEFAULT, H5P_DEFAULT) < 0)
        return fail(WFH5W_EIO, "copying %s failed", name);
    return WFH5W_OK;
}

static int make_table(wfh5w_out *o, const char *name, hid_t type) {
    close_table(o);
    const hsize_t dims[1] = {0}, maxdims[1] = {H5S_UNLIMITED}, chunk[1] = {CHUNK_ROWS};
    hid_t space = H5Screate_simple(1, dims, maxdims);
    hid_t plist = H5Pcreate(H5P_DATASET_CREATE);
    int rc = WFH5W_OK;
    if (space < 0 || plist < 0 || H5Pset_chunk(plist, 1, chunk) < 0 || H5Pset_deflate(plist, 9) < 0) {
        rc = fail(WFH5W_EIO, "cannot set up gzip-9 chunks for %s", name);
    } else {
        o->dset = H5Dcreate2(o->file, name, type, space, H5P_DEFAULT, plist, H5P_DEFAULT);
        if (o->dset < 0) rc = fail(WFH5W_EIO, "cannot create table %s", name);
    }
    if (plist >= 0) H5Pclose(plist);
    if (space >= 0) H5Sclose(space);
    if (rc == WFH5W_OK) {
        o->type = H5Tcopy(type);
        o->item_size = (int64_t)H5Tget_size(type);
    }
    return rc;
}

extern "C" int wfh5w_create_table_like(wfh5w_out *o, const wfh5w_in *in) {
    if (!o || !in) return fail(WFH5W_EINVAL, "NULL argument");
    quiet();
    return make_table(o, in->table.c_str(), in->type);
}

extern "C" int wfh5w_create_table(wfh5w_out *o, const char *name, const wfh5w_member *members, int32_t n_members,
                                  int64_t item_size) {
    if (!o || !name || !members) return fail(WFH5W_EINVAL, "NULL argument");
    if (n_members <= 0 || item_size <= 0) return fail(WFH5W_EINVAL, "%d members in %lld bytes", n_members, (long long)item_size);
    quiet();
    for (int i = 0; i < n_members; ++i) {
        const wfh5w_member &m = members[i];
        if (type_of(m.kind) < 0 || m.count <= 0 || m.offset < 0 || !memchr(m.name, 0, sizeof(m.name)) || !m.name[0] ||
            m.offset + (int64_t)size_of(m.kind) * m.count > item_size)
            return fail(WFH5W_EINVAL, "member %d is not described inside a record of %lld bytes", i, (long long)item_size);
        for (int j = 0; j < i; ++j) {
            const int64_t a0 = members[j].offset, a1 = a0 + (int64_t)size_of(members[j].kind) * members[j].count;
            if (m.offset < a1 && a0 < m.offset + (int64_t)size_of(m.kind) * m.count)
                return fail(WFH5W_EINVAL, "members %d and %d overlap", j, i);
        }
    }
    hid_t type = H5Tcreate(H5T_COMPOUND, (size_t)item_size);
    if (type < 0) return fail(WFH5W_EIO, "cannot create a compound type of %lld bytes", (long long)item_size);
    int rc = WFH5W_OK;
    for (int i = 0; i < n_members && rc == WFH5W_OK; ++i) {
        const wfh5w_member &m = members[i];
        hid_t mt;
        // the reference's numpy dtypes: ('<i4', (3,)) is an array member, '<i4' a scalar
        if (m.count > 1) {
            const hsize_t ad[1] = {(hsize_t)m.count};
            mt = H5Tarray_create2(type_of(m.kind), 1, ad);
        } else {
            mt = H5Tcopy(type_of(m.kind));
        }
        if (mt < 0 || H5Tinsert(type, m.name, (size_t)m.offset, mt) < 0) rc = fail(WFH5W_EIO, "cannot add member %s", m.name);
        if (mt >= 0) H5Tclose(mt);
    }
    if (rc == WFH5W_OK) rc = make_table(o, name, type);
    H5Tclose(type);
    return rc;
}

extern "C" int wfh5w_append(wfh5w_out *o, const void *records, int64_t n_rows) {
    if (!o || o->dset < 0) return fail(WFH5W_EINVAL, "no table to append to");
    if (n_rows < 0 || (n_rows > 0 && !records)) return fail(WFH5W_EINVAL, "%lld rows from %p", (long long)n_rows, records);
    if (n_rows == 0) return WFH5W_OK;
    quiet();
    const hsize_t size[1] = {(hsize_t)(o->rows + n_rows)}, start[1] = {(hsize_t)o->rows}, count[1] = {(hsize_t)n_rows};
    if (H5Dset_extent(o->dset, size) < 0) return fail(WFH5W_EIO, "cannot extend the table to %lld rows", (long long)size[0]);
    hid_t fspace = H5Dget_space(o->dset);
    hid_t mspace = H5Screate_simple(1, count, nullptr);
    int rc = WFH5W_OK;
    if (fspace < 0 || mspace < 0 || H5Sselect_hyperslab(fspace, H5S_SELECT_SET, start, nullptr, count, nullptr) < 0 ||
        H5Dwrite(o->dset, o->type, mspace, fspace, H5P_DEFAULT, records) < 0)
        rc = fail(WFH5W_EIO, "writing rows [%lld, %lld) failed", (long long)o->rows, (long long)size[0]);
    if (mspace >= 0) H5Sclose(mspace);
    if (fspace >= 0) H5Sclose(fspace);
    if (rc == WFH5W_OK) o->rows += n_rows;
    return rc;
}

extern "C" int wfh5w_flush(wfh5w_out *o) {
    if (!o) return fail(WFH5W_EINVAL, "NULL handle");
    quiet();
    if (H5Fflush(o->dset >= 0 ? o->dset : o->file, H5F_SCOPE_LOCAL) < 0) return fail(WFH5W_EIO, "flush failed");
    return WFH5W_OK;
}

// one attribute, type and dataspace as stored
static int copy_attr(hid_t from, hid_t to, const char *name) {
    hid_t a = H5Aopen(from, name, H5P_DEFAULT);
    if (a < 0) return fail(WFH5W_EIO, "cannot open attribute %s", name);
    hid_t t = H5Aget_type(a), s = H5Aget_space(a);
    int rc = WFH5W_OK;
    const hssize_t np = s >= 0 ? H5Sget_simple_extent_npoints(s) : -1;
    const size_t sz = t >= 0 ? H5Tget_size(t) : 0;
    if (t < 0 || np < 0 || sz == 0 || (uint64_t)np > (1u << 20) || sz > (1u << 20)) {
        rc = fail(WFH5W_EIO, "attribute %s cannot be described", name);
    } else {
        std::vector<char> buf((size_t)np * sz + 8, 0);
        if (H5Aexists(to, name) > 0) H5Adelete(to, name);
        hid_t b = -1;
        if (H5Aread(a, t, buf.data()) < 0) rc = fail(WFH5W_EIO, "cannot read attribute %s", name);
        else if ((b = H5Acreate2(to, name, t, s, H5P_DEFAULT, H5P_DEFAULT)) < 0 || H5Awrite(b, t, buf.data()) < 0)
            rc = fail(WFH5W_EIO, "cannot write attribute %s", name);
        if (b >= 0) H5Aclose(b);
        if (H5Tdetect_class(t, H5T_VLEN) > 0 || (H5Tget_class(t) == H5T_STRING && H5Tis_variable_str(t) > 0))
            H5Dvlen_reclaim(t, s, H5P_DEFAULT, buf.data());
    }
    if (s >= 0) H5Sclose(s);
    if (t >= 0) H5Tclose(t);
    H5Aclose(a);
    return rc;
}

extern "C" int wfh5w_copy_table_attrs(wfh5w_out *o, const wfh5w_in *in) {
    if (!o || !in || o->dset < 0) return fail(WFH5W_EINVAL, "no table to copy attributes to");
    quiet();
    std::vector<std::string> names = {"CLASS"};
    for (int n = 0; n < 4096; ++n) {
        char field[32];
        snprintf(field, sizeof(field), "FIELD_%d_NAME", n);
        if (H5Aexists(in->dset, field) <= 0) break;
        names.push_back(field);
    }
    for (const char *s : {"TITLE", "VERSION", "abstime", "runtime", "calgrp", "nevents", "rname", "scalingfactor"}) names.push_back(s);
    for (const std::string &n : names) {
        if (H5Aexists(in->dset, n.c_str()) <= 0) continue;          // an attribute the input lacks is skipped
        const int rc = copy_attr(in->dset, o->dset, n.c_str());
        if (rc != WFH5W_OK) return rc;
    }
    return WFH5W_OK;
}

extern "C" int wfh5w_set_attr_string(wfh5w_out *o, const char *name, const char *value) {
    if (!o || o->dset < 0 || !name || !value) return fail(WFH5W_EINVAL, "no table / NULL argument");
    quiet();
    hid_t t = H5Tcopy(H5T_C_S1), s = H5Screate(H5S_SCALAR), a = -1;
    int rc = WFH5W_OK;
    if (H5Aexists(o->dset, name) > 0) H5Adelete(o->dset, name);
    if (t < 0 || s < 0 || H5Tset_size(t, strlen(value) + 1) < 0 ||
        (a = H5Acreate2(o->dset, name, t, s, H5P_DEFAULT, H5P_DEFAULT)) < 0 || H5Awrite(a, t, value) < 0)
        rc = fail(WFH5W_EIO, "cannot write attribute %s", name);
    if (a >= 0) H5Aclose(a);
    if (s >= 0) H5Sclose(s);
    if (t >= 0) H5Tclose(t);
    return rc;
}

extern "C" int wfh5w_set_attr_f64(wfh5w_out *o, const char *name, double value) {
    if (!o || o->dset < 0 || !name) return fail(WFH5W_EINVAL, "no table / NULL argument");
    quiet();
    const hsize_t one[1] = {1};
    hid_t s = H5Screate_simple(1, one, nullptr), a = -1;
    int rc = WFH5W_OK;
    if (H5Aexists(o->dset, name) > 0) H5Adelete(o->dset, name);
    if (s < 0 || (a = H5Acreate2(o->dset, name, H5T_IEEE_F64LE, s, H5P_DEFAULT, H5P_DEFAULT)) < 0 ||
        H5Awrite(a, H5T_NATIVE_DOUBLE, &value) < 0)
        rc = fail(WFH5W_EIO, "cannot write attribute %s", name);
    if (a >= 0) H5Aclose(a);
    if (s >= 0) H5Sclose(s);
    return rc;
}
