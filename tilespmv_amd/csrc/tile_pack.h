// tile_pack.h — packing ONE tile of a Tile_matrix into its format's payload arrays (reference src/csr2tile.h:420-622; HYB index bytes :984-1008), written once for the host
// builder (host_tile_create.cpp) and the device builder (hip_tile_create.hip): both call THIS function, as both call select_format (tile_select.h).
// PRECONDITION: the tile's entries arrive in row order, and within a row in CSR order (the host's gather goes row by row; the device's sort is stable).  The walk below
// relies on it: it keeps the row it is in (rcur) and where that row started (rstart), and needs no per-row counts.
// DNS, DNSROW and DNSCOL have one slot per position: selection never gives them to a tile that stores a position twice (tile_select.h "repeated positions").
#pragma once
#include "host_util.h"

namespace tilespmv {

// where a tile's payload goes: the payload arrays of the Tile_matrix, and csr_col / ell_col, one byte per slot, which a pass over all tiles packs into the nibble streams
// csr_compressedIdx / ell_compressedIdx afterwards (two tiles may share a byte there).  hybIdx must be zero-filled: its nibbles are OR-ed in.
struct PackOut {
    val_t *Blockcsr_Val; unsigned char *Blockcsr_Ptr, *csr_col;
    val_t *Blockcoo_Val; unsigned char *coo_compressed_Idx;
    val_t *Blockell_Val; unsigned char *ell_col;
    val_t *Blockhyb_Val; unsigned char *hybIdx;
    val_t *Blockdense_Val, *Blockdenserow_Val; char *denserowid;
    val_t *Blockdensecol_Val; char *densecolid;
};
inline PackOut pack_out_of(const Tile_matrix &T, unsigned char *csr_col, unsigned char *ell_col)
{
    return {T.Blockcsr_Val, T.Blockcsr_Ptr, csr_col, T.Blockcoo_Val, T.coo_compressed_Idx, T.Blockell_Val, ell_col, T.Blockhyb_Val, T.hybIdx,
            T.Blockdense_Val, T.Blockdenserow_Val, T.denserowid, T.Blockdensecol_Val, T.densecolid};
}

// Tile t of T (its per-tile arrays selected and scanned), rowlen rows high; hyb_byte_off: a HYB tile's first byte in hybIdx.  rc(k): the (local row << 4) | local column
// byte of the tile's k-th entry; val(k): its value.  extract(slot, local_row, k) is called once per entry that also goes to the extracted matrix — every COO entry and
// every HYB remainder; slot counts from the tile's new_coocount.
template <class RcAt, class ValAt, class Extract>
TILESPMV_HD inline void pack_tile(const Tile_matrix &T, long long t, int rowlen, long long hyb_byte_off, RcAt rc, ValAt val, Extract extract, const PackOut &out)
{
    const int n = T.tile_nnz[t + 1] - T.tile_nnz[t];
    int rcur = 0, rstart = 0;   // the row the walk is in and where it starts
    switch (T.Format[t]) {
    case TILESPMV_FMT_CSR: {
        const int off = T.csr_offset[t], poff = T.csrptr_offset[t];
        out.Blockcsr_Ptr[poff] = 0;
        for (int k = 0; k < n; k++) {
            const int b = rc(k), r = b >> 4;
            while (rcur < r) { rcur++; if (rcur < rowlen) out.Blockcsr_Ptr[poff + rcur] = (unsigned char)k; }
            out.Blockcsr_Val[off + k] = val(k); out.csr_col[off + k] = (unsigned char)(b & 15);
        }
        while (rcur < rowlen - 1) { rcur++; out.Blockcsr_Ptr[poff + rcur] = (unsigned char)n; }   // trailing empty rows
        break;
    }
    case TILESPMV_FMT_COO: {
        const int off = T.coo_offset[t], xo = T.new_coocount[t];
        for (int k = 0; k < n; k++) {
            const int b = rc(k);
            out.Blockcoo_Val[off + k] = val(k);
            out.coo_compressed_Idx[off + k] = (unsigned char)b;
            extract(xo + k, b >> 4, k);
        }
        break;
    }
    case TILESPMV_FMT_ELL: {
        const int off = T.ell_offset[t];
        for (int k = 0; k < n; k++) {
            const int b = rc(k), r = b >> 4;
            if (r != rcur) { rcur = r; rstart = k; }
            const int p = off + (k - rstart) * rowlen + r;
            out.Blockell_Val[p] = val(k); out.ell_col[p] = (unsigned char)(b & 15);
        }
        break;
    }
    case TILESPMV_FMT_HYB: {   // ELL part of width w (slot-major, zero padded) + the entries beyond it in row order (src/csr2tile.h:505-548)
        const int off = T.hyb_offset[t], xo = T.new_coocount[t], w = T.tilewidth[t], nell = w * rowlen;
        unsigned char *ib = out.hybIdx + hyb_byte_off;   // this tile's bytes (nobody else's: the stream is tile-byte-aligned)
        int spill = 0;
        for (int k = 0; k < n; k++) {
            const int b = rc(k), r = b >> 4;
            if (r != rcur) { rcur = r; rstart = k; }
            const int sl = k - rstart;
            if (sl < w) {
                const int q = sl * rowlen + r;
                out.Blockhyb_Val[off + q] = val(k);
                ib[q >> 1] = (unsigned char)(ib[q >> 1] | ((q & 1) ? (b & 15) : ((b & 15) << 4)));   // nibble at position q of the tile's own stream: high nibble first
            } else {
                out.Blockhyb_Val[off + nell + spill] = val(k);
                ib[(nell + 1) / 2 + spill] = (unsigned char)b;   // (row << 4) | column
                extract(xo + spill, r, k);
                spill++;
            }
        }
        break;
    }
    case TILESPMV_FMT_DNS: {
        const int off = T.dns_offset[t];
        for (int k = 0; k < n; k++) { const int b = rc(k); out.Blockdense_Val[off + (b & 15) * rowlen + (b >> 4)] = val(k); }
        break;
    }
    case TILESPMV_FMT_DNSROW: {   // every occupied row is a full row: the values of the full rows back to back, their row ids in order
        const int off = T.dnsrow_offset[t], ro = T.dnsrowptr[t];
        int nr = 0, last = -1;
        for (int k = 0; k < n; k++) {
            const int r = rc(k) >> 4;
            if (r != last) { out.denserowid[ro + nr++] = (char)r; last = r; }
            out.Blockdenserow_Val[off + k] = val(k);
        }
        break;
    }
    case TILESPMV_FMT_DNSCOL: {
        const int off = T.dnscol_offset[t], co = T.dnscolptr[t];
        for (int k = 0; k < n; k++) {
            const int b = rc(k), r = b >> 4;
            if (r != rcur) { rcur = r; rstart = k; }
            if (r == 0) out.densecolid[co + k] = (char)(b & 15);   // the columns present = the columns of row 0
            out.Blockdensecol_Val[off + (k - rstart) * rowlen + r] = val(k);
        }
        break;
    }
    default: break;
    }
}

}  // namespace tilespmv
