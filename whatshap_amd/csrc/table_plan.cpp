// table_plan.cpp -- see table_plan.h.
#include "table_plan.h"

#include <cstring>

namespace whamd {

GroupVariantPair group_variants_of(const SlotBatchEntry& he, bool ped) {
	if (ped) {
		const GroupVariant v = he.ex.nf == (uint32_t)PSLOT_FACT4 ? GV_QUARTET_FACT : he.ex.nf == (uint32_t)PSLOT_FACT ? GV_TRIO_FACT : he.ex.nf == 16 ? GV_PED_2_16
		                       : he.ex.tb == 4 ? (he.ex.nf == 4 ? GV_PED_4_4 : GV_PED_4_2) : (he.ex.nf == 4 ? GV_PED_2_4 : GV_PED_2_2);
		return {v, v};
	}
	const GroupVariant v = he.run.lr == 3 ? GV_SINGLE8 : GV_SINGLE4;
	return {v, (he.run.yflags & 8u) ? (he.run.lr == 3 ? GV_X8 : GV_X4) : v};
}

void append_segments(uint32_t mask, std::vector<uint32_t>& out, uint16_t& count) {
	uint32_t src = 0;
	count = 0;
	for (uint32_t bit = 0; bit < 32;) {
		if (!((mask >> bit) & 1u)) { ++bit; continue; }
		uint32_t len = 0;
		while (bit + len < 32 && ((mask >> (bit + len)) & 1u)) ++len;
		out.push_back(src | (bit << 8) | (len << 16));
		++count;
		src += len;
		bit += len;
	}
}

uint32_t preview_pieces_of(uint32_t wanted, uint32_t n_pieces) { return wanted ? wanted : std::max(1u, n_pieces / 6); }

// What a column's descriptor holds by itself, and its 32-bit term offsets (b.term_ptr32): a few host threads.  Fails if the problem exceeds 32-bit offsets.  Host only.
whamd_status_t describe_columns(const Problem& p, TableBuild& b, TablePlan& m, std::string& msg) {
	const uint32_t n = b.n, ni = b.ni, tbits = b.tbits;
	if (p.terms.size() >= 0xFFFFFFFFull || (uint64_t)p.col_ptr[n] * ni >= 0xFFFFFFFFull) {
		msg = "problem too large for 32-bit device offsets";
		return WHAMD_ERR_UNSUPPORTED;
	}
	m.cols.resize(n);
	b.term_ptr32.resize((size_t)n * (p.T + 1));
	RawVec<uint32_t>& term_ptr32 = b.term_ptr32;
	parallel_ranges(n, host_threads(n, 16384), [&m, &p, &term_ptr32, n, ni, tbits](uint64_t c0, uint64_t c1, uint32_t) {
		for (uint32_t c = (uint32_t)c0; c < (uint32_t)c1; ++c) {
			DevColumn d{};
			d.k = p.k[c];
			d.b = p.b[c];
			d.f = p.f[c];
			d.recomb = p.recomb[c];
			d.delta_off = (uint32_t)(p.col_ptr[c] * ni);
			d.term_off = (uint32_t)((size_t)c * (p.T + 1));
			for (uint32_t t = 0; t <= p.T; ++t) term_ptr32[(size_t)c * (p.T + 1) + t] = (uint32_t)p.term_ptr[(size_t)c * p.T + t];
			d.ebits = d.k - d.f;
			d.is_last = (c + 1 == n);
			d.eloop = std::min<uint32_t>(d.ebits, QMAX);
			d.nplanes = d.ebits + tbits;
			m.cols[c] = d;
		}
	});
	return WHAMD_OK;
}

uint32_t column_step_mode(bool force_keys, bool is_last, uint32_t f, uint32_t ebits) { return (!force_keys && !is_last && f >= 6 && ebits <= (uint32_t)QMAX) ? 0u : 1u; }
uint64_t column_record_bytes(uint32_t mode, uint32_t T, uint32_t f, uint32_t nplanes) {
	return mode == 0 ? (uint64_t)nplanes * T * (1ull << (f - 6)) * 8ull : (uint64_t)T * (1ull << f) * 4ull;
}
uint64_t arena_capacity(uint64_t free_b, uint32_t n, uint64_t table_bytes, uint64_t arena_limit) {
	const uint64_t reserve = (3ull << 30) + (uint64_t)n * 1024ull + table_bytes;
	uint64_t cap = free_b > reserve ? free_b - reserve : 0;
	if (arena_limit) cap = std::min<uint64_t>(cap, arena_limit);
	return cap;
}
uint64_t arena_behind(uint64_t bt, uint64_t bytes) { return (bt + bytes + 15ull) & ~15ull; }
uint64_t slot_run_record_bytes(const SlotRun& run) { return (uint64_t)run.n_ends * run.threads * (1ull << (run.g - run.half)); }

// The offsets that run through the table, in column order: segment lists (b.segs), the place of every backtrace unit's record in the arena (DevColumn::bt_off, the
// runs' rec / bt words), the windows where the arena is smaller than the records (b.window_first_col).  Produces b.arena_cap, b.bt, b.max_f, b.max_keys_f,
// b.exchange_bytes; fails if a unit or the whole does not fit.  Host only.
whamd_status_t lay_out_arena(const Problem& p, const TableOptions& o, TableBuild& b, TablePlan& m, std::string& msg) {
	const uint32_t n = b.n;
	const bool ped_slots = b.ped_slots;
	std::vector<uint32_t>& segs = b.segs;
	uint64_t bt = 0, seg_bt = 0;
	size_t seg_cursor = 0, slot_cursor = 0;
	uint32_t max_f = 0, max_keys_f = 0;
	auto slot_record_bytes = [&m, ped_slots](size_t ri) -> uint64_t {   // record of one slot run: only launched workgroups write
		const SlotRun& run = m.splan.runs[ri];
		if (ped_slots) return (uint64_t)m.splan.pextra[ri].rec_words * 4ull << run.g;
		return slot_run_record_bytes(run);
	};
	const uint64_t arena_cap = arena_capacity(b.free_b, n, m.table_bytes, o.arena_limit);
	b.arena_cap = arena_cap;
	std::vector<uint32_t>& window_first_col = b.window_first_col;
	uint64_t bt_max = 0;
	auto open_unit = [&bt, &bt_max, &window_first_col, arena_cap](uint32_t c, uint64_t bytes) -> bool {   // a backtrace unit of `bytes` starts at column c
		if (bytes + 16 > arena_cap) return false;
		if (bt + bytes + 16 > arena_cap) {
			bt_max = std::max(bt_max, bt);
			bt = 0;
			window_first_col.push_back(c);
		}
		return true;
	};
	auto unit_too_large = [&msg, &b](uint32_t c) {
		msg = "the backtrace record of the unit at column " + std::to_string(c) + " alone does not fit in the arena (" + std::to_string(b.arena_cap >> 20) +
		      " MiB of " + std::to_string(b.free_b >> 20) + " MiB free HBM)";
		return WHAMD_ERR_UNSUPPORTED;
	};
	for (uint32_t c = 0; c < n; ++c) {
		DevColumn& d = m.cols[c];
		const bool in_slot_run = m.use_slots && m.splan.col_to_row[c] >= 0;   // (the run kernels read none of the per-column arrays)
		d.seg_off = (uint32_t)segs.size();
		const uint32_t kmask = d.k >= 32 ? 0xFFFFFFFFu : ((1u << d.k) - 1u);
		if (!in_slot_run) {
			append_segments(p.fwd_mask[c], segs, d.nseg_fwd);
			append_segments(kmask & ~p.fwd_mask[c], segs, d.nseg_end);
		}
		d.bt_off = bt;
		if (m.use_slots && m.splan.col_to_row[c] >= 0) {
			d.mode = 3;
			d.res_idx = (uint32_t)m.splan.col_to_row[c];
			if (slot_cursor < m.splan.runs.size() && m.splan.runs[slot_cursor].c0 == c) {  // first column of a slot run
				SlotRun& run = m.splan.runs[slot_cursor];
				if (!open_unit(c, slot_record_bytes(slot_cursor))) return unit_too_large(c);
				run.rec_lo = (uint32_t)bt;
				run.rec_hi = (uint32_t)(bt >> 32);
				seg_bt = bt;
				bt += slot_record_bytes(slot_cursor);
				max_f = std::max(max_f, run.L + run.g);   // entry / exit indices in physical order need 2^(L + g) entries
				++slot_cursor;
			}
			d.bt_off = seg_bt;
		} else if (m.plan.col_to_res[c] >= 0) {
			d.mode = 2;
			d.res_idx = (uint32_t)m.plan.col_to_res[c];
			if (seg_cursor < m.plan.segments.size() && m.plan.segments[seg_cursor].c0 == c) {  // first column of a run
				ResSegment& sgm = m.plan.segments[seg_cursor];
				if (!open_unit(c, (uint64_t)sgm.stage_words * (1ull << sgm.g) * 8ull)) return unit_too_large(c);
				sgm.bt_lo = (uint32_t)bt;
				sgm.bt_hi = (uint32_t)(bt >> 32);
				seg_bt = bt;
				bt += (uint64_t)sgm.stage_words * (1ull << sgm.g) * 8ull;
				++seg_cursor;
			}
			d.bt_off = seg_bt;
		} else {
			d.mode = column_step_mode(b.force_keys, d.is_last, d.f, d.ebits);
			const uint64_t bytes = column_record_bytes(d.mode, p.T, d.f, d.nplanes);
			if (!open_unit(c, bytes)) return unit_too_large(c);
			d.bt_off = bt;
			bt += bytes;
			if (d.mode != 0) max_keys_f = std::max(max_keys_f, d.f);
		}
		bt = (bt + 15ull) & ~15ull;
		max_f = std::max(max_f, d.f);
	}
	b.laps.lap("column descriptors (host)");
	bt = std::max(bt_max, bt);
	b.bt = bt;
	b.max_f = max_f;
	b.max_keys_f = max_keys_f;
	b.exchange_bytes = (size_t)(1ull << max_f) * p.T * 4;
	m.bt_bytes = bt;
	m.windowed = !window_first_col.empty();
	m.checkpoint_bytes = b.exchange_bytes;
	const uint64_t need = bt + (2ull + window_first_col.size()) * b.exchange_bytes + (1ull << max_keys_f) * p.T * 8ull;
	if (need + (1ull << 30) > b.free_b) {
		msg = "backtrace arena of " + std::to_string(need >> 20) + " MiB does not fit in free HBM (" + std::to_string(b.free_b >> 20) + " MiB)";
		return WHAMD_ERR_UNSUPPORTED;
	}
	return WHAMD_OK;
}

// An upper bound of what the phases below hand to TableUploader::up (the size of the table's device block and staging image).
size_t upload_bound(const Problem& p, const TableBuild& b, const TablePlan& m) {
	const size_t delta_count = p.n_ind == 0 ? std::max<size_t>(p.col_ptr[b.n], 1) : (size_t)p.col_ptr[b.n] * p.n_ind;
	const size_t super_upload = m.device_superreads ? ((size_t)b.n + 1) * 8 + b.n + 1024 : 0;
	return m.cols.size() * sizeof(DevColumn) + delta_count * sizeof(int32_t) + b.term_ptr32.size() * 4 + (p.terms.size() + p.fterms.size()) * sizeof(DevTerm) + b.segs.size() * 4 +
	       m.plan.columns.size() * (sizeof(ResColumn) + sizeof(ResBacktrace) + sizeof(PedColumn)) + m.plan.ped_terms.size() * sizeof(PedTerm) +
	       (m.splan.rows.size() + SLOT_ROW_PAD) * sizeof(SlotRow) + m.splan.prows.size() * sizeof(PedSlotRow) + m.splan.bt_cols.size() * (sizeof(SlotBtCol) + 8) +
	       m.splan.runs.size() * (sizeof(SlotRun) + sizeof(PedSlotExtra) + sizeof(BtUnit) + sizeof(SlotBatchEntry) + 64) + m.plan.segments.size() * (sizeof(ResBatchEntry) + sizeof(BtUnit)) + super_upload + ((size_t)8 << 20);
}

// Slot runs: the backtrace blob ([ncols] SlotBtCol + ending slots per run) and where every run's piece lies in it (b.slot_blob_off / _words).  Host only.
void build_slot_blobs(const TablePlan& m, TableBuild& b) {
	b.slot_blob_off.assign(m.splan.runs.size(), 0);
	b.slot_blob_words.assign(m.splan.runs.size(), 0);
	// offsets first (one pass over the runs), then every run copies its own piece (8 MB for configs[2]: 0.9 ms when it was one growing vector)
	size_t words = 0;
	for (size_t ri = 0; ri < m.splan.runs.size(); ++ri) {
		const SlotRun& run = m.splan.runs[ri];
		b.slot_blob_off[ri] = (uint32_t)words;
		b.slot_blob_words[ri] = (uint32_t)((size_t)run.ncols * (sizeof(SlotBtCol) / 4) + (run.n_ends + 3) / 4 + 1);
		words += b.slot_blob_words[ri];
	}
	b.slot_blob.resize(words);
	uint32_t* blob = b.slot_blob.data();
	const uint32_t* blob_off = b.slot_blob_off.data();
	parallel_ranges(m.splan.runs.size(), host_threads(m.splan.runs.size(), 512), [&m, blob, blob_off](uint64_t r0, uint64_t r1, uint32_t) {
		for (size_t ri = r0; ri < r1; ++ri) {
			const SlotRun& run = m.splan.runs[ri];
			uint32_t* dst = blob + blob_off[ri];
			const size_t col_words = (size_t)run.ncols * (sizeof(SlotBtCol) / 4);
			std::memcpy(dst, m.splan.bt_cols.data() + run.row_off, col_words * 4);
			const size_t end_words = (run.n_ends + 3) / 4 + 1;
			std::memset(dst + col_words, 0, end_words * 4);
			if (run.n_ends) std::memcpy(dst + col_words, m.splan.end_slots.data() + m.splan.end_off[ri], run.n_ends);
		}
	});
}

// Single-individual slot runs: where the prologue's tables of every run (SlotRun::tab_g / tab_w / tab_sl, an X run's tab_kr / tab_par) lie in the table block that
// slot_tables fills; marks the X runs.  Returns the block's size in words.  Host only, and the same on every call (the preview lays the tables out before the create does).
uint64_t lay_out_slot_tables(TablePlan& m, const TableBuild& b, bool report) {
	uint64_t slot_tab_words = 0;
	for (SlotRun& run : m.splan.runs) {
		auto pad4 = [](uint64_t v) { return (v + 3ull) & ~3ull; };
		// X runs (kernels_slots.h, slot_runx_body): a Y-form run with four cells per thread whose columns and ending reads fit the kernel's registers; the
		// rows of its tables are padded with zero columns to a pair of trips
		const bool xrun = (run.yflags & 1u) && (run.lr == 2u || (run.lr == 3u && !debug_env("WHAMD_NO_XRUN8"))) && run.ncols <= (uint32_t)SLOT_XCOLS &&
		                  run.n_ends <= (uint32_t)SLOT_XENDS && !debug_env("WHAMD_NO_XRUN");
		const uint64_t ncp = xrun ? ((run.ncols + 7u) & ~7u) : run.ncols;
		run.tab_g = (uint32_t)slot_tab_words;
		slot_tab_words += pad4(ncp << (run.g - run.half));
		run.tab_w = (uint32_t)slot_tab_words;
		slot_tab_words += pad4(ncp * (run.threads >> 6));
		run.tab_sl = (uint32_t)slot_tab_words;
		slot_tab_words += ncp * 64u;
		if (xrun) {
			run.yflags |= 8u;
			slot_tab_words = (slot_tab_words + 15u) & ~(uint64_t)15;   // (a trip's sixteen Kr words are ONE 64-byte line of the scalar cache)
			run.tab_kr = (uint32_t)slot_tab_words;
			slot_tab_words += pad4((((uint64_t)run.ncols + SLOT_XPAD) << run.lr) + run.ncols + SLOT_XPAD);   // Kr words, then one control word per column
			run.tab_par = (uint32_t)slot_tab_words;
			slot_tab_words += pad4((uint64_t)run.threads + (1ull << (run.g - run.half)));
		}
	}
	slot_tab_words += (uint64_t)SLOT_XCOLS * 64u;   // (an X run requests the lane parts of SLOT_XCOLS columns whatever its length)
	if (b.laps.on && report) {
		size_t nx = 0, not_y = 0, not_lr = 0, long_run = 0, many_ends = 0;
		for (const SlotRun& run : m.splan.runs) {
			nx += (run.yflags & 8u) != 0;
			not_y += !(run.yflags & 1u); not_lr += run.lr != 2u && run.lr != 3u; long_run += run.ncols > (uint32_t)SLOT_XCOLS; many_ends += run.n_ends > (uint32_t)SLOT_XENDS;
		}
		fprintf(stderr, "[whamd timing]   X runs: %zu of %zu (not Y form %zu, cells per thread %zu, more than %d columns %zu, more than %d ending reads %zu)\n", nx, m.splan.runs.size(), not_y,
		        not_lr, SLOT_XCOLS, long_run, SLOT_XENDS, many_ends);
	}
	return slot_tab_words;
}

// Jobs (see Job): connected components made of runs only get their own job.  Host only.
void make_jobs(const TableOptions& o, TablePlan& m) {
	Job final_job;
	final_job.final = true;
	std::vector<Job> component_jobs;
	const std::vector<uint32_t>& first = m.plan.component_first_step;
	// Components as jobs of their own run side by side on lanes -- and walk back one after the other through the SEQUENTIAL backtrace (the chunked one takes a
	// single job): 16 ms for an irregular coverage-20 table of 200 000 columns whose forward pass is 57 ms, nearly all of it one giant component (a Poisson layout
	// leaves a gap every few ten thousand columns).  A table whose largest component holds four fifths of its steps or more stays ONE job: the lanes would gain
	// less than the walk loses ((1 - s) x forward against s x 16 ms).  WHAMD_SPLIT_COMPONENTS=1 (debug library): always split, as before.
	size_t largest = 0;
	for (size_t k = 0; k < first.size(); ++k) largest = std::max<size_t>(largest, (k + 1 < first.size() ? first[k + 1] : m.plan.steps.size()) - first[k]);
	const bool worth_splitting = largest * 5 < m.plan.steps.size() * 4 || debug_env("WHAMD_SPLIT_COMPONENTS");
	const bool split = o.max_lanes > 1 && first.size() > 1 && worth_splitting && !debug_env("WHAMD_DEBUG_STAMPS") && !m.windowed;
	if (!split) {
		for (uint32_t si = 0; si < m.plan.steps.size(); ++si) final_job.steps.push_back(si);
	} else {
		for (size_t k = 0; k < first.size(); ++k) {
			const uint32_t s0 = first[k], s1 = k + 1 < first.size() ? first[k + 1] : (uint32_t)m.plan.steps.size();
			Job* job = &final_job;
			if (k + 1 < first.size()) { component_jobs.emplace_back(); job = &component_jobs.back(); }
			for (uint32_t si = s0; si < s1; ++si) job->steps.push_back(si);
		}
	}
	m.jobs.push_back(std::move(final_job));
	for (Job& j : component_jobs) m.jobs.push_back(std::move(j));
}

// The backtrace units: every job's steps in reverse order, each with everything the walk needs of it.  Reads b.segs, b.slot_blob_off / _words.  Host only.
void make_units(const TableBuild& b, TablePlan& m) {
	m.units.clear();
	for (Job& job : m.jobs) {
		job.unit_off = (uint32_t)m.units.size();
		for (size_t sj = job.steps.size(); sj-- > 0;) {
			const Step& st = m.plan.steps[job.steps[sj]];
			BtUnit u{};
			u.kind = st.kind;
			if (st.kind == 0) {
				// column step: everything the backtrace needs, so that its chain holds no descriptor load
				const DevColumn& d = m.cols[st.index];
				u.c0 = st.index;
				u.ncols = 1;
				u.g = d.f; u.Lf_last = d.mode; u.stage_words = d.nplanes; u.n_wext = d.ebits;
				u.bt_lo = (uint32_t)d.bt_off; u.bt_hi = (uint32_t)(d.bt_off >> 32);
				u.n_lext = d.nseg_fwd; u.pad0 = d.nseg_end;
				const uint32_t nseg = (uint32_t)d.nseg_fwd + d.nseg_end;
				if (nseg <= (uint32_t)(RES_IOSEG + RES_BT_LRUNS)) {
					uint32_t* dst = u.wext;  // wext[6] and lext[10] are contiguous: 16 run slots
					for (uint32_t i = 0; i < nseg; ++i) dst[i] = b.segs[d.seg_off + i];
					u.pad1[0] = 1;  // runs are inline
				}
			} else if (st.kind == 2) {
				const SlotRun& run = m.splan.runs[st.index];
				SlotBtUnit su{};
				su.kind = b.ped_slots ? 3 : 2; su.c0 = run.c0; su.ncols = run.ncols; su.blob_off = b.slot_blob_off[st.index];
				su.g = run.g; su.L = run.L; su.n_ends = run.n_ends; su.threads = run.threads;
				su.bt_lo = run.rec_lo; su.bt_hi = run.rec_hi; su.half = run.half; su.blob_words = b.slot_blob_words[st.index];
				su.f_exit = m.splan.f_exit[st.index];
				for (uint32_t j = 0; j < su.f_exit && j < 32; ++j) su.exit_pos[j] = (uint8_t)slot_pos(run.out_pos, m.splan.exit_slot[st.index][j]);
				su.lr = run.lr;
				if (b.ped_slots) { su.n_ends = m.splan.pextra[st.index].rec_words; su.lr = m.splan.pextra[st.index].tb; }   // kind 3: words of one workgroup's record, log2 T
				for (uint32_t j = 0; j < su.f_exit && j < 32; ++j) su.exit_slot[j] = m.splan.exit_slot[st.index][j];
				static_assert(sizeof(SlotBtUnit) == sizeof(BtUnit), "unit headers share one array");
				std::memcpy(&u, &su, sizeof u);
			} else {
				const ResSegment& sgm = m.plan.segments[st.index];
				u.c0 = sgm.c0; u.ncols = sgm.ncols; u.col_off = sgm.col_off; u.g = sgm.g; u.Lf_last = sgm.Lf_last;
				u.stage_words = sgm.stage_words; u.n_wext = sgm.n_wext; u.bt_lo = sgm.bt_lo; u.bt_hi = sgm.bt_hi;
				u.n_lext = sgm.n_lext;
				u.pad0 = (uint32_t)sgm.bt_active | ((uint32_t)sgm.bt_simple << 16) | (sgm.half << 20);
				std::copy(sgm.wext, sgm.wext + RES_IOSEG, u.wext);
				std::copy(sgm.lext, sgm.lext + RES_BT_LRUNS, u.lext);
			}
			m.units.push_back(u);
		}
		job.unit_count = (uint32_t)m.units.size() - job.unit_off;
	}
}

// Windows (see Window) of a windowed table: the single job's steps cut where the arena offsets start over (b.window_first_col), and their backtrace jobs.  Host only.
whamd_status_t cut_windows(const TableBuild& b, TablePlan& m, std::vector<BtJob>& wjobs, std::string& msg) {
	const std::vector<uint32_t>& window_first_col = b.window_first_col;
	const std::vector<uint32_t>& steps = m.jobs[0].steps;
	const uint32_t n_steps = (uint32_t)steps.size();
	auto first_col = [&m, &steps](uint32_t pos) {
		const Step& st = m.plan.steps[steps[pos]];
		return st.kind == 0 ? st.index : (st.kind == 2 ? m.splan.runs[st.index].c0 : m.plan.segments[st.index].c0);
	};
	Window w;
	size_t next = 0;
	for (uint32_t pos = 0; pos < n_steps; ++pos) {
		if (next < window_first_col.size() && first_col(pos) == window_first_col[next]) {
			w.step_hi = pos;
			m.windows.push_back(w);
			w = Window();
			w.step_lo = pos;
			++next;
		}
	}
	w.step_hi = n_steps;
	m.windows.push_back(w);
	if (next != window_first_col.size()) { msg = "internal error: a window does not start at a step"; return WHAMD_ERR_DEVICE; }
	wjobs.clear();
	for (size_t wi = 0; wi < m.windows.size(); ++wi) {   // units are the steps in reverse order
		Window& win = m.windows[wi];
		win.unit_off = n_steps - win.step_hi;
		win.unit_count = win.step_hi - win.step_lo;
		wjobs.push_back(BtJob{win.unit_off, win.unit_count, wi + 1 == m.windows.size() ? 1u : 2u, 0u});
	}
	return WHAMD_OK;
}

namespace {

// Orientation generators of the speculative backtrace (BtChunk): per individual the transmission bits its relabelling flips -- a founder those of the
// trios it is a parent of, a child both of its own trio (exact where genotypes are heterozygous); individuals that are
// both, or pedigrees with more than BT_GENERATORS individuals, get no generator (still exact, more walked twice).  Pure in the problem.
struct OrientationGenerators {
	std::vector<int> of_individual;   // -1: none
	std::vector<uint32_t> tflip;
	explicit OrientationGenerators(const Problem& p) : of_individual(std::max<uint32_t>(p.n_ind, 1), -1) {
		if (p.n_ind < 2 || p.n_ind > BT_GENERATORS) return;
		for (uint32_t s = 0; s < p.n_ind; ++s) {
			uint32_t as_parent = 0, as_child = 0;
			for (uint32_t t3 = 0; t3 < p.n_triples; ++t3) {
				if (p.triples[t3][0] == s) as_parent |= 1u << (2 * t3);
				if (p.triples[t3][1] == s) as_parent |= 1u << (2 * t3 + 1);
				if (p.triples[t3][2] == s) as_child |= 3u << (2 * t3);
			}
			if (as_parent && as_child) continue;
			if (!as_parent && !as_child) continue;   // unrelated individual of a multi-sample table
			of_individual[s] = (int)tflip.size();
			tflip.push_back(as_parent | as_child);
		}
	}
	// the orientations of a chunk that starts from the projection column of column c_last: bit j = j-th forwarded read
	void orient(const Problem& p, uint32_t c_last, BtChunk& ch) const {
		ch.n_orient = 1;
		for (uint32_t q = 0; q < BT_GENERATORS; ++q) ch.flip[q] = 0;
		if (p.n_triples == 0 && p.n_ind <= 1) {
			const uint32_t fb = p.f[c_last];
			ch.flip[0] = fb >= BT_STATE_TSHIFT ? BT_STATE_XMASK : ((1u << fb) - 1u);
			ch.n_orient = 2;
			return;
		}
		if (tflip.empty()) return;
		const ColumnEntry* col = p.col_begin(c_last);
		uint32_t bit = 0;
		for (uint32_t j = 0; j < p.k[c_last]; ++j) {
			if (!((p.fwd_mask[c_last] >> j) & 1u)) continue;
			const int gq = of_individual[col[j].sample];
			if (gq >= 0) ch.flip[gq] |= 1u << bit;
			++bit;
		}
		for (size_t q = 0; q < tflip.size(); ++q) ch.flip[q] |= tflip[q] << BT_STATE_TSHIFT;
		ch.n_orient = 1u << tflip.size();
	}
};

}  // namespace

bool backtrace_is_chunked(bool on_runs, size_t n_jobs, bool windowed, size_t n_units) {
	return on_runs && n_jobs == 1 && !windowed && !getenv("WHAMD_BT_SEQUENTIAL") && n_units > 2u * BT_CHUNK_RUNS;
}
uint32_t seed_stride_of(uint32_t stride, const SlotRun& run) { return std::max(stride, (run.threads >> 6) << (run.g - run.half)); }

// Chunks of the speculative backtrace (single job only); the run that leaves a chunk's seed gets its spec id.  Host only.
// Produces m.use_chunks, m.chunks, m.n_spec, m.n_orient_max and, where the table is chunked, spec_stride (DevProblem::spec_stride).
void cut_chunks(const Problem& p, TablePlan& m, uint32_t& spec_stride) {
	m.use_chunks = false;
	m.chunks.clear();
	m.n_spec = 0;
	for (SlotRun& run : m.splan.runs) run.spec_id = 0;
	const bool trio_runs = !m.use_slots && !m.plan.ped_columns.empty();   // LDS-resident trio runs (kernels_trio.h)
	if (trio_runs) for (ResSegment& sgm : m.plan.segments) sgm.in_mirror_bit = 0;   // (trio runs have no mirror: the field carries the spec id)
	if (!backtrace_is_chunked(m.use_slots || trio_runs, m.jobs.size(), m.windowed, m.units.size())) return;
	m.use_chunks = true;
	const OrientationGenerators generators(p);
	BtChunk first{};
	first.n_orient = 1;   // the newest chunk starts from the table's optimum
	m.chunks.push_back(first);
	m.n_spec = cut_chunk_starts(m.units.size(),
		[&m, trio_runs](size_t u) { return m.units[u].kind == 2 || m.units[u].kind == 3 || (trio_runs && m.units[u].kind == 1); },
		[&m, &p, &generators, trio_runs](size_t u, uint32_t id) {
			m.chunks.back().unit_count = (uint32_t)u - m.chunks.back().unit_off;
			BtChunk cur{};
			cur.unit_off = (uint32_t)u;
			cur.spec_id = id;
			generators.orient(p, m.units[u].c0 + m.units[u].ncols - 1, cur);   // (the last column of unit u's step)
			m.chunks.push_back(cur);
			// the run of unit u leaves the seed: units are the job's steps in reverse order
			const Step& st = m.plan.steps[m.jobs[0].steps[m.jobs[0].steps.size() - 1 - u]];
			if (trio_runs) m.plan.segments[st.index].in_mirror_bit = id;
			else m.splan.runs[st.index].spec_id = id;
		});
	m.chunks.back().unit_count = (uint32_t)m.units.size() - m.chunks.back().unit_off;
	m.n_orient_max = 1;
	for (const BtChunk& ch : m.chunks) m.n_orient_max = std::max(m.n_orient_max, ch.n_orient);
	uint32_t stride = 64;
	for (const SlotRun& run : m.splan.runs) if (run.spec_id) stride = seed_stride_of(stride, run);
	if (trio_runs) for (const ResSegment& sgm : m.plan.segments) if (sgm.in_mirror_bit) stride = std::max(stride, (sgm.threads >> 6) << sgm.g);
	spec_stride = stride;
}

// The LDS sizes of the two backtrace kernels (backtrace_kernel, backtrace_chunks): their fixed areas and the largest record any unit stages.  Host only.
void backtrace_lds_sizes(const TableBuild& b, TablePlan& m) {
	uint32_t max_stage = 0;
	for (const ResSegment& sgm : m.plan.segments) max_stage = std::max(max_stage, sgm.stage_words);
	for (size_t ri = 0; ri < m.splan.runs.size(); ++ri)
		max_stage = std::max(max_stage, b.ped_slots ? m.splan.pextra[ri].rec_words / 2u : (m.splan.runs[ri].n_ends * m.splan.runs[ri].threads + 7) / 8);
	m.bt_lds = (size_t)2 * RES_MAXCOLS * 128 + 512 + 16 + (size_t)BT_CELLS * 4 + (size_t)RES_MAXCOLS * 4 + (size_t)max_stage * 8 + 16;
	m.chunk_lds = (size_t)(32 + 4 + BT_CELLS + BT_CHUNK_BLOB) * 4 + (size_t)max_stage * 8 + 16;
}

// Lanes: longest job first to the least loaded lane; lane 0 always runs the final job.  (The driver gives every lane its buffers.)  Host only.
void assign_lanes(const TableOptions& o, const TableBuild& b, TablePlan& m) {
	// at most 1 GiB of private exchange buffers (coverage 23: 64 MiB per lane)
	const size_t lane_bytes = 2 * b.exchange_bytes;
	const size_t by_memory = std::max<size_t>(1, ((size_t)1 << 30) / std::max<size_t>(lane_bytes, 1));
	const size_t n_lanes = std::max<size_t>(1, std::min<size_t>(std::min<size_t>((size_t)o.max_lanes, by_memory), m.jobs.size()));
	m.lanes.assign(n_lanes, Lane());
	std::vector<uint64_t> load(n_lanes, 0);
	std::vector<uint32_t> order;
	for (uint32_t j = 1; j < m.jobs.size(); ++j) order.push_back(j);
	std::stable_sort(order.begin(), order.end(), [&m](uint32_t x, uint32_t y) { return m.jobs[x].steps.size() > m.jobs[y].steps.size(); });
	m.lanes[0].jobs.push_back(0);
	load[0] = m.jobs[0].steps.size() + 1;
	for (uint32_t j : order) {
		const size_t l = (size_t)(std::min_element(load.begin(), load.end()) - load.begin());
		m.lanes[l].jobs.push_back(j);
		load[l] += m.jobs[j].steps.size() + 1;
	}
}

// The schedule: the lanes advance in lockstep; super-step t holds step t of every lane that still has one.  Makes the entries of the batched launches
// (m.entries / m.slot_entries: they carry the device pointers of the lanes' buffers, of d_job_scores and of `dp`) and, windowed, the replay of every older
// window.  Host only.
whamd_status_t make_schedule(const TableBuild& b, const DevProblem& dp, uint32_t* d_job_scores, TablePlan& m, std::string& msg) {
	const bool ped_slots = b.ped_slots;
	struct Cursor { size_t job_i = 0, step_i = 0; uint32_t flip = 0; };
	std::vector<Cursor> cur(m.lanes.size());
	for (;;) {
		SuperStep ss;
		ss.entry_off = (uint32_t)(m.use_slots ? m.slot_entries.size() : m.entries.size());
		for (size_t li = 0; li < m.lanes.size(); ++li) {
			Lane& lane = m.lanes[li];
			Cursor& c = cur[li];
			if (c.job_i == lane.jobs.size()) continue;
			const uint32_t job_id = lane.jobs[c.job_i];
			const Job& job = m.jobs[job_id];
			const uint32_t si = job.steps[c.step_i];
			const bool first = c.step_i == 0, last = c.step_i + 1 == job.steps.size();
			const Step& step = m.plan.steps[si];
			ss.io[0] = lane.d_pr[c.flip]; ss.io[1] = lane.d_pr[c.flip ^ 1];
			if (step.kind == 2) {
				SlotBatchEntry e{};
				e.run = m.splan.runs[step.index];
				if (first) e.run.has_prev = 0;  // a job starts from cost 0
				e.prev = lane.d_pr[c.flip];
				e.cur = lane.d_pr[c.flip ^ 1];
				e.score_out = (last && !job.final) ? d_job_scores + job_id : nullptr;
				if (m.splan.ped) {
					const PedSlotExtra& pex = m.splan.pextra[step.index];
					ss.lds = std::max<size_t>(ss.lds, pedslot_lds_bytes(e.run.threads, e.run.ncols, pex));
				} else
				ss.lds = std::max<size_t>(ss.lds, slot_run_lds_bytes(e.run.threads, e.run.lr, e.run.ncols));
				e.pad = step.index;
				// the owning table's arrays: a group launch (slot_group / pedslot_group) serves runs of several tables
				if (ped_slots) e.ex = m.splan.pextra[step.index];
				e.tab = ped_slots ? dp.pslot_tab : dp.slot_tab;
				e.rows = ped_slots ? (const void*)dp.pslot_rows : (const void*)dp.slot_rows;
				e.ctrl = dp.slot_ctrl;
				e.bt = dp.bt;
				e.spec_keys = dp.spec_keys;
				e.spec_stride = dp.spec_stride;
				if (const char* skip = debug_env("WHAMD_SLOT_SKIP")) e.pad2 = (uint32_t)atoi(skip);   // (timing experiments in a group launch)
				if (debug_env("WHAMD_NO_WARM")) e.pad2 |= 0x10000u;
				ss.grid_x = std::max(ss.grid_x, 1u << (e.run.g - e.run.half));
				ss.threads = std::max(ss.threads, e.run.threads);
				m.slot_entries.push_back(e);
				++ss.entry_count;
			} else if (step.kind == 1) {
				ResBatchEntry e{};
				e.sg = m.plan.segments[step.index];
				e.sg.pad = step.index;
				if (first) e.sg.has_prev = 0;  // a job starts from cost 0
				e.prev = lane.d_pr[c.flip];
				e.cur = lane.d_pr[c.flip ^ 1];
				e.score_out = (last && !job.final) ? d_job_scores + job_id : nullptr;
				ss.lds = std::max<size_t>(ss.lds, res_segment_lds_bytes(e.sg));
				ss.grid_x = std::max(ss.grid_x, 1u << (e.sg.g - e.sg.half));
				ss.threads = std::max(ss.threads, e.sg.threads);
				ss.sym = ss.sym || e.sg.half || e.sg.in_half || e.sg.mirror_out;
				m.entries.push_back(e);
				++ss.entry_count;
			} else {
				ss.singles.push_back(Single{(uint32_t)li, si, c.flip, first, (last && !job.final) ? (int32_t)job_id : -1});
			}
			c.flip ^= 1;
			if (last) { ++c.job_i; c.step_i = 0; } else ++c.step_i;
		}
		if (!ss.entry_count && ss.singles.empty()) break;
		m.max_grid_x = std::max(m.max_grid_x, ss.grid_x * std::max(1u, ss.entry_count));
		m.schedule.push_back(std::move(ss));
	}
	if (m.windowed) {
		// one lane, one job: super-step i is step i.  Pass 1 = the schedule as it is, plus the kept columns and the
		// walk of the newest window; then every older window again, newest first.
		if (m.schedule.size() != m.jobs[0].steps.size()) { msg = "internal error: windowed schedule"; return WHAMD_ERR_DEVICE; }
		const size_t nw = m.windows.size();
		for (size_t wi = 0; wi + 1 < nw; ++wi) m.schedule[m.windows[wi].step_hi - 1].ck_save = (int32_t)wi;
		m.schedule.back().bt_window = (int32_t)(nw - 1);
		for (size_t wi = nw - 1; wi-- > 0;) {
			const Window& win = m.windows[wi];
			for (uint32_t pos = win.step_lo; pos < win.step_hi; ++pos) {
				SuperStep again = m.schedule[pos];
				again.ck_save = -1;
				again.ck_load = (pos == win.step_lo && wi > 0) ? (int32_t)(wi - 1) : -1;
				again.bt_window = pos + 1 == win.step_hi ? (int32_t)wi : -1;
				m.schedule.push_back(std::move(again));
			}
		}
	}
	return WHAMD_OK;
}

// What a group submission reads of the schedule (see StepBrief / EntryBrief).  Host only.
void make_briefs(TablePlan& m) {
	m.step_brief.clear();
	m.entry_brief.clear();
	if (!m.use_slots) return;
	m.step_brief.reserve(m.schedule.size());
	m.entry_brief.reserve(m.slot_entries.size());
	for (const SuperStep& ss : m.schedule) {
		m.step_brief.push_back(StepBrief{(uint32_t)m.entry_brief.size(), (uint32_t)ss.lds, (uint16_t)ss.entry_count, (uint8_t)(ss.singles.empty() ? 0 : 1), 0});
		for (uint32_t q = 0; q < ss.entry_count; ++q) {
			const SlotBatchEntry& he = m.slot_entries[ss.entry_off + q];
			EntryBrief eb{};
			eb.grid_x = (uint16_t)(1u << (he.run.g - he.run.half));
			eb.threads = (uint16_t)he.run.threads;
			eb.lds_x = (uint32_t)((size_t)2 * he.run.threads * (4u << he.run.lr));
			eb.variant = group_variants_of(he, m.splan.ped);
			m.entry_brief.push_back(eb);
		}
	}
}

// Which steps a preview would launch and what each is given by value, worked out ahead of the phases that normally produce it.  Host only (the debug library's
// whamd_debug_preview_plan holds it against lay_out_arena and cut_chunks without a device).  out.why says whether there is one: the table's form, the options,
// and -- under `auto` -- that the table is alone (`alone`: the driver counts the tables of a device).  The record offsets are the sum lay_out_arena will make, from
// its own helpers; the seeds' ids come from the chunk rule cut_chunks walks (cut_chunk_starts), here over the plan's steps.
void plan_preview(const Problem& p, const TableOptions& o, const TableBuild& b, TablePlan& m, bool from_create, bool alone, PreviewPlan& out) {
	const uint32_t n = b.n, n_pieces = slot_plan_pieces(n);
	out = PreviewPlan();
	auto none = [&out](uint32_t why) { out.why = why; };
	if (o.preview_mode == 0 || debug_env("WHAMD_NO_PREVIEW")) return none(PV_OFF);
	if (!from_create) return none(PV_NOT_CREATE);
	if (!m.use_slots || m.splan.ped || p.T != 1) return none(PV_NOT_SLOTS);
	if (debug_env("WHAMD_DEBUG_STAMPS") || debug_env("WHAMD_SLOT_STAMPS") || debug_env("WHAMD_SLOT_SKIP")) return none(PV_DEBUG_SWITCH);
	if (o.shared_hint || o.side_by_side) return none(PV_SHARED);
	if (m.plan.component_first_step.size() != 1) return none(PV_COMPONENTS);
	if (n_pieces < 2) return none(PV_FEW_PIECES);
	if (o.preview_mode < 0) {   // auto: only where a speculative forward pass competes with nothing
		if (o.thread_budget) return none(PV_THREAD_BUDGET);
		if (n_pieces < 8) return none(PV_FEW_PIECES);
		if (!alone) return none(PV_NOT_ALONE);
	}
	out.pieces = std::min(n_pieces - 1, preview_pieces_of(o.preview_pieces, n_pieces));
	const uint32_t col_limit = slot_plan_piece_begin(n, out.pieces);
	// ---- the leading steps that are slot runs inside the pieces (a piece edge is a run boundary)
	const std::vector<Step>& steps = m.plan.steps;
	const std::vector<SlotRun>& runs = m.splan.runs;
	uint32_t S = 0;
	while (S < steps.size() && steps[S].kind == 2 && steps[S].index == S && runs[S].c0 + runs[S].ncols <= col_limit) ++S;
	if (S == 0 || S >= steps.size()) return none(PV_NO_LEADING_RUNS);
	out.end_col = runs[S - 1].c0 + runs[S - 1].ncols;
	if ((size_t)out.end_col + SLOT_ROW_PAD > m.splan.rows.size()) return none(PV_ROW_PAD);   // (a run's scalar-cache warm-up touches a fixed number of rows behind its own)
	// ---- what the runs carry by value: table offsets, record offsets, the ids of the seeds they leave
	const uint64_t tab_words_all = lay_out_slot_tables(m, b, false);
	out.tab_words = (S < runs.size() ? runs[S].tab_g : tab_words_all) + (uint64_t)SLOT_XCOLS * 64u;   // (lay_out_slot_tables: the slack an X run may request)
	out.ctrl_words = (size_t)runs[S - 1].ctrl_off + SLOT_CTRL_WORDS;
	if (tab_words_all >= 0xFFFFFFFFull || out.ctrl_words > m.splan.ctrl.size()) return none(PV_NO_LEADING_RUNS);
	out.rec.assign(S, 0);
	uint64_t bt = 0;
	{
		// the records of ALL steps, in order, as lay_out_arena places them when they fit one window (arena_capacity, arena_behind, the record sizes: its own)
		const uint64_t cap = arena_capacity(b.free_b, n, m.table_bytes, o.arena_limit);
		for (size_t k = 0; k < steps.size(); ++k) {
			uint64_t bytes = 0;
			if (steps[k].kind == 2) bytes = slot_run_record_bytes(runs[steps[k].index]);
			else {
				const uint32_t c = steps[k].index, f = p.f[c], ebits = p.k[c] - f;
				bytes = column_record_bytes(column_step_mode(b.force_keys, c + 1 == n, f, ebits), p.T, f, ebits + b.tbits);
			}
			if (bt + bytes + 16 > cap) return none(PV_ARENA);   // (windowed, or too large altogether)
			if (k < S) out.rec[k] = bt;
			bt = arena_behind(bt, bytes);
		}
		if (bt + (1ull << 31) > b.free_b) return none(PV_ARENA);
	}
	out.arena = bt;
	out.spec.assign(S, 0);
	out.stride = 64;
	out.chunked = backtrace_is_chunked(true, 1, false, steps.size());   // (one job of slot runs, not windowed: checked above)
	if (out.chunked)
		out.n_spec = cut_chunk_starts(steps.size(), [&steps](size_t u) { return steps[steps.size() - 1 - u].kind == 2; },
			[&](size_t u, uint32_t id) {
				const size_t k = steps.size() - 1 - u;
				out.stride = seed_stride_of(out.stride, runs[steps[k].index]);
				if (k < S) out.spec[k] = id;
			});
	out.max_f = p.max_k;   // (a bound of the widest exchange column: no column forwards more reads than it has, a run's entries are 2^(L + g))
	for (const SlotRun& run : runs) out.max_f = std::max(out.max_f, run.L + run.g);
	out.steps = S;
	out.why = PV_RAN;
}

}  // namespace whamd
