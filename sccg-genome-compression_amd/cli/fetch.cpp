// fetch -- `fetch <record_file> <reference_file> <region>...`: regions of the target read from an
// extracted compressed_genome.txt (no 7z call) without rebuilding it (sccg_reader_*).  A region is
// `begin-end`, 1-based and inclusive as in `samtools faidx`, or a bare `pos` (one base).  Per region
// it prints `>name:begin-end` (name: the record's header line without its '>', `seq` when it has
// none) and the bases wrapped at 50 columns (decompression.cpp:266-274's width).  All regions go in
// one sccg_reader_fetch call.  `fetch -i <record_file> <reference_file> <region>...` (also
// --reverse-complement; recognised as the first argument only) prints every region reverse-
// complemented, as `samtools faidx -i` does, with `/rc` appended to its header line.  Exit code 1 on
// usage / region / open / format errors; the regions are parsed before the GPU is touched.
// `fetch --origin <record_file> <reference_file> <region>...` (first argument only) prints, per
// region, the usual header line and then where its bases come from (sccg_reader_segments, through a
// reference opened with SCCG_REF_COORDS): one tab-separated line per maximal run, everything 1-based
// and inclusive -- `tbegin tend rbegin rend` for bases copied from consecutively ascending reference
// positions, `tbegin tend *` for literals of the record line, `tbegin tend N` for bases of the target's
// N runs.  --origin together with -i is a usage error.
// `fetch --locate ...` and `fetch --lift ...` (first argument only) ask the other way round, from the
// reference to the sequence: locate_main and lift_main below.
// `fetch --find <PATTERN> ...` (first argument only) asks where an IUPAC pattern occurs: find_main below;
// `fetch --find-approx <K> <PATTERN> ...` where it occurs within K substitutions: find_approx_main.
#include "cli_common.h"

#include <cstring>

// decimal digits only, no sign, fits int64
static bool parse_pos(const std::string& s, int64_t* v) {
    if (s.empty() || s.size() > 18) return false;
    int64_t x = 0;
    for (char c : s) {
        if (c < '0' || c > '9') return false;
        x = x * 10 + (c - '0');
    }
    *v = x;
    return true;
}

// `fetch --locate <record_file> <reference_file> <refpos>...`: one line per query, `refpos pos copies`
// tab-separated, 1-based; pos is `-` when no token copies the position and `N` inside an erased N run
static int locate_main(int argc, char* argv[]) {
    const bool mixed = argc > 2 && (std::string(argv[2]) == "-i" || std::string(argv[2]) == "--reverse-complement" ||
                                    std::string(argv[2]) == "--origin" || std::string(argv[2]) == "--lift" ||
                                    std::string(argv[2]) == "--find");
    if (argc < 5 || mixed) {
        std::cerr << "Usage: " << argv[0] << " --locate <record_file> <reference_file> <refpos>...\n"
                  << "  refpos: a 1-based position of the reference sequence; prints refpos, the first 1-based sequence\n"
                  << "  position holding a copy of it (- none, N an erased reference N) and the number of copies\n"
                  << "  --locate is the first argument only, not with -i or --origin\n";
        return 1;
    }
    std::vector<int64_t> q;
    for (int i = 4; i < argc; i++) {
        int64_t v = 0;
        if (!parse_pos(argv[i], &v) || v < 1) {
            std::cerr << "Error: malformed reference position '" << argv[i] << "' (1-based, decimal)\n";
            return 1;
        }
        q.push_back(v - 1);
    }
    std::string ref, rec;
    if (!slurp(argv[3], ref)) {
        std::cerr << "Greska pri otvaranju reference: " << argv[3] << "\n";
        return 1;
    }
    if (!slurp(argv[2], rec)) {
        std::cerr << "Greska pri otvaranju datoteke: " << argv[2] << "\n";
        return 1;
    }
    sccg_ctx* ctx = nullptr;
    int rc = sccg_ctx_create(cli_device(), &ctx);
    if (rc) {
        std::cerr << "Error: no usable GPU (sccg_ctx_create rc=" << rc << ")\n";
        return 1;
    }
    sccg_reference* rf = nullptr;
    sccg_reader* rd = nullptr;
    rc = sccg_reference_open(ctx, ref.data(), ref.size(), SCCG_REF_COORDS, &rf);
    if (!rc) rc = sccg_reader_open_shared(rf, rec.data(), rec.size(), &rd);
    sccg_reference_close(rf);
    if (!rc) rc = sccg_reader_enable_locate(rd);
    std::vector<int64_t> pos(q.size());
    std::vector<int32_t> copies(q.size());
    if (!rc) rc = sccg_reader_locate(rd, q.data(), q.size(), pos.data(), copies.data());
    if (rc) {
        std::cerr << "Error locating: " << sccg_last_error(ctx) << " (rc=" << rc << ")\n";
        sccg_reader_close(rd);
        sccg_ctx_destroy(ctx);
        return 1;
    }
    std::string out;
    for (size_t i = 0; i < q.size(); i++)
        out += std::to_string(q[i] + 1) + "\t" +
               (pos[i] == SCCG_LOCATE_REF_N ? std::string("N") : pos[i] < 0 ? std::string("-") : std::to_string(pos[i] + 1)) + "\t" +
               std::to_string(copies[i]) + "\n";
    std::cout << out;
    sccg_reader_close(rd);
    sccg_ctx_destroy(ctx);
    return 0;
}

// `fetch --lift <record_file> <reference_file> <refregion>...`: per region of the reference sequence
// (`begin-end`, 1-based inclusive, or a bare `pos`) a line `>begin-end`, then one tab-separated line per
// block (sccg_reader_lift), everything 1-based and inclusive: `rbegin rend tbegin tend` for reference bases
// that lie at consecutively ascending sequence positions, `rbegin rend -` where no token copies them,
// `rbegin rend N` for an erased N run of the reference
static int lift_main(int argc, char* argv[]) {
    const std::string a2 = argc > 2 ? argv[2] : "";
    const bool mixed = a2 == "-i" || a2 == "--reverse-complement" || a2 == "--origin" || a2 == "--locate" || a2 == "--find";
    if (argc < 5 || mixed) {
        std::cerr << "Usage: " << argv[0] << " --lift <record_file> <reference_file> <refregion>...\n"
                  << "  refregion: begin-end (1-based, inclusive) or pos, of the reference sequence; prints >begin-end, then\n"
                  << "  one line per block: rbegin rend tbegin tend (where the bases lie in the sequence) | rbegin rend -\n"
                  << "  (no copy) | rbegin rend N (an erased reference N run)\n"
                  << "  --lift is the first argument only, not with -i, --origin or --locate\n";
        return 1;
    }
    std::vector<sccg_region> iv;
    for (int i = 4; i < argc; i++) {
        const std::string a = argv[i];
        const size_t dash = a.find('-');
        int64_t b = 0, e = 0;
        const bool ok = dash == std::string::npos ? parse_pos(a, &b) && (e = b, true)
                                                  : parse_pos(a.substr(0, dash), &b) && parse_pos(a.substr(dash + 1), &e);
        if (!ok || b < 1 || e < b) {
            std::cerr << "Error: malformed reference region '" << a << "' (begin-end, 1-based, inclusive, begin <= end)\n";
            return 1;
        }
        iv.push_back(sccg_region{b - 1, e});
    }
    std::string ref, rec;
    if (!slurp(argv[3], ref)) {
        std::cerr << "Greska pri otvaranju reference: " << argv[3] << "\n";
        return 1;
    }
    if (!slurp(argv[2], rec)) {
        std::cerr << "Greska pri otvaranju datoteke: " << argv[2] << "\n";
        return 1;
    }
    sccg_ctx* ctx = nullptr;
    int rc = sccg_ctx_create(cli_device(), &ctx);
    if (rc) {
        std::cerr << "Error: no usable GPU (sccg_ctx_create rc=" << rc << ")\n";
        return 1;
    }
    sccg_reference* rf = nullptr;
    sccg_reader* rd = nullptr;
    rc = sccg_reference_open(ctx, ref.data(), ref.size(), SCCG_REF_COORDS, &rf);
    if (!rc) rc = sccg_reader_open_shared(rf, rec.data(), rec.size(), &rd);
    sccg_reference_close(rf);
    if (!rc) rc = sccg_reader_enable_locate(rd);
    sccg_buf blk{};
    std::vector<int64_t> off(iv.size() + 1);
    if (!rc) rc = sccg_reader_lift(rd, iv.data(), iv.size(), off.data(), &blk);
    if (rc) {
        std::cerr << "Error lifting: " << sccg_last_error(ctx) << " (rc=" << rc << ")\n";
        sccg_reader_close(rd);
        sccg_ctx_destroy(ctx);
        return 1;
    }
    std::string out;
    for (size_t i = 0; i < iv.size(); i++) {
        out += ">" + std::to_string(iv[i].begin + 1) + "-" + std::to_string(iv[i].end) + "\n";
        for (int64_t k = off[i]; k < off[i + 1]; k++) {
            sccg_lift_block g;
            memcpy(&g, blk.data + (size_t)k * sizeof g, sizeof g);
            out += std::to_string(g.ref + 1) + "\t" + std::to_string(g.ref + g.len) + "\t";
            if (g.pos >= 0) out += std::to_string(g.pos + 1) + "\t" + std::to_string(g.pos + g.len);
            else out += g.pos == SCCG_LOCATE_REF_N ? "N" : "-";
            out += '\n';
        }
    }
    std::cout << out;
    sccg_buf_free(&blk);
    sccg_reader_close(rd);
    sccg_ctx_destroy(ctx);
    return 0;
}

// `fetch --find <PATTERN> <record_file> <reference_file> <region>...`: per region of the sequence (`begin-end`,
// 1-based inclusive, or a bare `pos`) a line `>begin-end`, then one tab-separated line per hit of the IUPAC
// pattern on either strand (sccg_reader_find): `pos strand bases` -- pos the 1-based leftmost position of the
// window, strand `+` or `-`, bases the window as the sample carries it, forward strand (one ordinary fetch
// of all hit windows).  A malformed pattern is a usage error before the GPU is touched.
static int find_main(int argc, char* argv[]) {
    const std::string pat = argc > 2 ? argv[2] : "";
    const bool mixed = pat == "-i" || pat == "--reverse-complement" || pat == "--origin" || pat == "--locate" || pat == "--lift" ||
                       pat == "--find";
    const bool bad_pattern = argc > 2 && !mixed && sccg_find_pattern_masks(pat.data(), pat.size(), nullptr, nullptr) != SCCG_OK;
    if (argc < 6 || mixed || bad_pattern) {
        if (bad_pattern)
            std::cerr << "Error: malformed pattern '" << pat << "' (1 to " << SCCG_FIND_MAX_PATTERN
                      << " IUPAC nucleotide letters, ACGTURYSWKMBDHVN in either case)\n";
        std::cerr << "Usage: " << argv[0] << " --find <PATTERN> <record_file> <reference_file> <region>...\n"
                  << "  PATTERN: 1 to " << SCCG_FIND_MAX_PATTERN << " IUPAC nucleotide letters (N: any of A, C, G, T); both strands are searched\n"
                  << "  region: begin-end (1-based, inclusive) or pos; prints >begin-end, then one line per hit:\n"
                  << "      pos strand(+|-) bases -- the window's leftmost position and its bases on the forward strand\n"
                  << "  --find is the first argument only, not with -i, --origin, --locate or --lift\n";
        return 1;
    }
    std::vector<sccg_region> regions;
    for (int i = 5; i < argc; i++) {
        const std::string a = argv[i];
        const size_t dash = a.find('-');
        int64_t b = 0, e = 0;
        const bool ok = dash == std::string::npos ? parse_pos(a, &b) && (e = b, true)
                                                  : parse_pos(a.substr(0, dash), &b) && parse_pos(a.substr(dash + 1), &e);
        if (!ok || b < 1 || e < b) {
            std::cerr << "Error: malformed region '" << a << "' (begin-end, 1-based, inclusive, begin <= end)\n";
            return 1;
        }
        regions.push_back(sccg_region{b - 1, e});
    }
    std::string ref, rec;
    if (!slurp(argv[4], ref)) {
        std::cerr << "Greska pri otvaranju reference: " << argv[4] << "\n";
        return 1;
    }
    if (!slurp(argv[3], rec)) {
        std::cerr << "Greska pri otvaranju datoteke: " << argv[3] << "\n";
        return 1;
    }
    sccg_ctx* ctx = nullptr;
    int rc = sccg_ctx_create(cli_device(), &ctx);
    if (rc) {
        std::cerr << "Error: no usable GPU (sccg_ctx_create rc=" << rc << ")\n";
        return 1;
    }
    sccg_reader* rd = nullptr;
    rc = sccg_reader_open(ctx, ref.data(), ref.size(), rec.data(), rec.size(), &rd);
    if (rc) {
        std::cerr << "Error opening the record: " << sccg_last_error(ctx) << " (rc=" << rc << ")\n";
        sccg_ctx_destroy(ctx);
        return 1;
    }
    sccg_buf hits{}, bases{};
    std::vector<int64_t> off(regions.size() + 1);
    std::vector<sccg_hit> hit;
    rc = sccg_reader_find(rd, pat.data(), pat.size(), regions.data(), regions.size(), SCCG_FIND_FWD | SCCG_FIND_REV, off.data(), &hits);
    if (!rc) {   // the windows of all hits in one fetch
        hit.resize(hits.len / sizeof(sccg_hit));
        if (!hit.empty()) memcpy(hit.data(), hits.data, hit.size() * sizeof(sccg_hit));
        std::vector<sccg_region> win(hit.size());
        for (size_t k = 0; k < hit.size(); k++) win[k] = sccg_region{hit[k].pos, hit[k].pos + (int64_t)pat.size()};
        rc = sccg_reader_fetch(rd, win.data(), win.size(), 0, &bases);
    }
    if (rc) {
        std::cerr << "Error finding: " << sccg_last_error(ctx) << " (rc=" << rc << ")\n";
        sccg_buf_free(&hits);
        sccg_reader_close(rd);
        sccg_ctx_destroy(ctx);
        return 1;
    }
    std::string out;
    for (size_t i = 0; i < regions.size(); i++) {
        out += ">" + std::to_string(regions[i].begin + 1) + "-" + std::to_string(regions[i].end) + "\n";
        for (int64_t k = off[i]; k < off[i + 1]; k++) {
            out += std::to_string(hit[(size_t)k].pos + 1) + "\t" + (hit[(size_t)k].strand ? "-" : "+") + "\t";
            out.append(bases.data + (size_t)k * pat.size(), pat.size());
            out += '\n';
        }
    }
    std::cout << out;
    sccg_buf_free(&hits);
    sccg_buf_free(&bases);
    sccg_reader_close(rd);
    sccg_ctx_destroy(ctx);
    return 0;
}

// `fetch --find-approx <K> <PATTERN> <record_file> <reference_file> <region>...`: find_main with up to K
// substitutions (sccg_reader_find_approx): per region `>begin-end`, then `pos strand mismatches bases` per hit.
// K is decimal, at most SCCG_FIND_MAX_MISMATCHES and less than the pattern's length; a malformed K, pattern or
// region is a usage error before the GPU is touched.
static int find_approx_main(int argc, char* argv[]) {
    const std::string ks = argc > 2 ? argv[2] : "", pat = argc > 3 ? argv[3] : "";
    const auto is_flag = [](const std::string& a) {
        return a == "-i" || a == "--reverse-complement" || a == "--origin" || a == "--locate" || a == "--lift" || a == "--find" ||
               a == "--find-approx";
    };
    const bool mixed = is_flag(ks) || is_flag(pat);
    std::string err;
    int64_t K = 0;
    std::vector<sccg_region> regions;
    if (argc >= 7 && !mixed) {
        if (sccg_find_pattern_masks(pat.data(), pat.size(), nullptr, nullptr) != SCCG_OK)
            err = "malformed pattern '" + pat + "' (1 to " + std::to_string(SCCG_FIND_MAX_PATTERN) +
                  " IUPAC nucleotide letters, ACGTURYSWKMBDHVN in either case)";
        else if (!parse_pos(ks, &K) || K > SCCG_FIND_MAX_MISMATCHES || K >= (int64_t)pat.size())
            err = "malformed mismatches '" + ks + "' (decimal, 0 to " + std::to_string(SCCG_FIND_MAX_MISMATCHES) +
                  " and less than the pattern's " + std::to_string(pat.size()) + " letters)";
        for (int i = 6; i < argc && err.empty(); i++) {
            const std::string a = argv[i];
            const size_t dash = a.find('-');
            int64_t b = 0, e = 0;
            const bool ok = dash == std::string::npos ? parse_pos(a, &b) && (e = b, true)
                                                      : parse_pos(a.substr(0, dash), &b) && parse_pos(a.substr(dash + 1), &e);
            if (!ok || b < 1 || e < b) err = "malformed region '" + a + "' (begin-end, 1-based, inclusive, begin <= end)";
            regions.push_back(sccg_region{b - 1, e});
        }
    }
    if (argc < 7 || mixed || !err.empty()) {
        if (!err.empty()) std::cerr << "Error: " << err << "\n";
        std::cerr << "Usage: " << argv[0] << " --find-approx <K> <PATTERN> <record_file> <reference_file> <region>...\n"
                  << "  K: substitutions allowed, 0 to " << SCCG_FIND_MAX_MISMATCHES << " and less than the pattern's length\n"
                  << "  PATTERN: 1 to " << SCCG_FIND_MAX_PATTERN << " IUPAC nucleotide letters (N: any of A, C, G, T); both strands are searched;\n"
                  << "      a sequence base that is not A, C, G or T is a mismatch against every letter\n"
                  << "  region: begin-end (1-based, inclusive) or pos; prints >begin-end, then one line per hit:\n"
                  << "      pos strand(+|-) mismatches bases -- the window's leftmost position and its bases on the forward strand\n"
                  << "  --find-approx is the first argument only, not with -i, --origin, --locate, --lift or --find\n";
        return 1;
    }
    std::string ref, rec;
    if (!slurp(argv[5], ref)) {
        std::cerr << "Greska pri otvaranju reference: " << argv[5] << "\n";
        return 1;
    }
    if (!slurp(argv[4], rec)) {
        std::cerr << "Greska pri otvaranju datoteke: " << argv[4] << "\n";
        return 1;
    }
    sccg_ctx* ctx = nullptr;
    int rc = sccg_ctx_create(cli_device(), &ctx);
    if (rc) {
        std::cerr << "Error: no usable GPU (sccg_ctx_create rc=" << rc << ")\n";
        return 1;
    }
    sccg_reader* rd = nullptr;
    rc = sccg_reader_open(ctx, ref.data(), ref.size(), rec.data(), rec.size(), &rd);
    if (rc) {
        std::cerr << "Error opening the record: " << sccg_last_error(ctx) << " (rc=" << rc << ")\n";
        sccg_ctx_destroy(ctx);
        return 1;
    }
    sccg_buf hits{}, bases{};
    std::vector<int64_t> off(regions.size() + 1);
    std::vector<sccg_hit_mm> hit;
    rc = sccg_reader_find_approx(rd, pat.data(), pat.size(), regions.data(), regions.size(), SCCG_FIND_FWD | SCCG_FIND_REV, (uint32_t)K,
                                 off.data(), &hits);
    if (!rc) {   // the windows of all hits in one fetch
        hit.resize(hits.len / sizeof(sccg_hit_mm));
        if (!hit.empty()) memcpy(hit.data(), hits.data, hit.size() * sizeof(sccg_hit_mm));
        std::vector<sccg_region> win(hit.size());
        for (size_t k = 0; k < hit.size(); k++) win[k] = sccg_region{hit[k].pos, hit[k].pos + (int64_t)pat.size()};
        rc = sccg_reader_fetch(rd, win.data(), win.size(), 0, &bases);
    }
    if (rc) {
        std::cerr << "Error finding: " << sccg_last_error(ctx) << " (rc=" << rc << ")\n";
        sccg_buf_free(&hits);
        sccg_reader_close(rd);
        sccg_ctx_destroy(ctx);
        return 1;
    }
    std::string out;
    for (size_t i = 0; i < regions.size(); i++) {
        out += ">" + std::to_string(regions[i].begin + 1) + "-" + std::to_string(regions[i].end) + "\n";
        for (int64_t k = off[i]; k < off[i + 1]; k++) {
            const sccg_hit_mm& h = hit[(size_t)k];
            out += std::to_string(h.pos + 1) + "\t" + (h.strand ? "-" : "+") + "\t" + std::to_string(h.mismatches) + "\t";
            out.append(bases.data + (size_t)k * pat.size(), pat.size());
            out += '\n';
        }
    }
    std::cout << out;
    sccg_buf_free(&hits);
    sccg_buf_free(&bases);
    sccg_reader_close(rd);
    sccg_ctx_destroy(ctx);
    return 0;
}

int main(int argc, char* argv[]) {
    if (argc > 1 && std::string(argv[1]) == "--find-approx") return find_approx_main(argc, argv);
    if (argc > 1 && std::string(argv[1]) == "--find") return find_main(argc, argv);
    if (argc > 1 && std::string(argv[1]) == "--lift") return lift_main(argc, argv);
    if (argc > 1 && std::string(argv[1]) == "--locate") return locate_main(argc, argv);
    const bool rc_flag = argc > 1 && (std::string(argv[1]) == "-i" || std::string(argv[1]) == "--reverse-complement");
    const bool origin = argc > 1 && std::string(argv[1]) == "--origin";
    const int a0 = rc_flag || origin ? 2 : 1;   // the first file argument
    const bool both = argc > 2 && ((origin && (std::string(argv[2]) == "-i" || std::string(argv[2]) == "--reverse-complement")) ||
                                   (rc_flag && std::string(argv[2]) == "--origin") ||
                                   ((origin || rc_flag) && (std::string(argv[2]) == "--lift" || std::string(argv[2]) == "--find")));
    if (argc < a0 + 3 || both) {
        std::cerr << "Usage: " << argv[0] << " [-i | --origin] <record_file> <reference_file> <region>...\n"
                  << "  region: begin-end (1-based, inclusive) or pos\n"
                  << "  -i, --reverse-complement (first argument only): every region reverse-complemented\n"
                  << "  --origin (first argument only, not with -i): where each base comes from, one line per run:\n"
                  << "      tbegin tend rbegin rend (copied from the reference) | tbegin tend * (literal) | tbegin tend N\n";
        return 1;
    }
    const std::string rec_path = argv[a0], ref_path = argv[a0 + 1];
    std::vector<sccg_region> regions;
    for (int i = a0 + 2; i < argc; i++) {
        const std::string a = argv[i];
        const size_t dash = a.find('-');
        int64_t b = 0, e = 0;
        const bool ok = dash == std::string::npos ? parse_pos(a, &b) && (e = b, true)
                                                  : parse_pos(a.substr(0, dash), &b) && parse_pos(a.substr(dash + 1), &e);
        if (!ok || b < 1 || e < b) {
            std::cerr << "Error: malformed region '" << a << "' (begin-end, 1-based, inclusive, begin <= end)\n";
            return 1;
        }
        regions.push_back(sccg_region{b - 1, e});
    }
    std::string ref, rec;
    if (!slurp(ref_path, ref)) {
        std::cerr << "Greska pri otvaranju reference: " << ref_path << "\n";
        return 1;
    }
    if (!slurp(rec_path, rec)) {
        std::cerr << "Greska pri otvaranju datoteke: " << rec_path << "\n";
        return 1;
    }
    sccg_ctx* ctx = nullptr;
    int rc = sccg_ctx_create(cli_device(), &ctx);
    if (rc) {
        std::cerr << "Error: no usable GPU (sccg_ctx_create rc=" << rc << ")\n";
        return 1;
    }
    sccg_reader* rd = nullptr;
    if (origin) {   // through a reference that keeps the R' -> R map; the reader holds it from here on
        sccg_reference* rf = nullptr;
        rc = sccg_reference_open(ctx, ref.data(), ref.size(), SCCG_REF_COORDS, &rf);
        if (!rc) rc = sccg_reader_open_shared(rf, rec.data(), rec.size(), &rd);
        sccg_reference_close(rf);
    } else {
        rc = sccg_reader_open(ctx, ref.data(), ref.size(), rec.data(), rec.size(), &rd);
    }
    if (rc) {
        std::cerr << "Error opening the record: " << sccg_last_error(ctx) << " (rc=" << rc << ")\n";
        sccg_ctx_destroy(ctx);
        return 1;
    }
    sccg_buf seq{};
    std::vector<int64_t> seg_off(regions.size() + 1);
    if (origin) {   // the maximal runs themselves: seq holds sccg_segment[]
        rc = sccg_reader_segments(rd, regions.data(), regions.size(), seg_off.data(), &seq);
    } else if (rc_flag) {
        const sccg_fetch_format fmt{SCCG_ENC_ASCII, SCCG_DT_U8, SCCG_FETCH_REVCOMP, 0};
        rc = sccg_reader_fetch_encoded(rd, regions.data(), regions.size(), nullptr, &fmt, &seq);
    } else {
        rc = sccg_reader_fetch(rd, regions.data(), regions.size(), 0, &seq);
    }
    if (rc) {
        std::cerr << "Error fetching: " << sccg_last_error(ctx) << " (rc=" << rc << ")\n";
        sccg_reader_close(rd);
        sccg_ctx_destroy(ctx);
        return 1;
    }
    size_t hlen = 0;
    const char* hdr = sccg_reader_header(rd, &hlen);
    const std::string name = hlen > 1 ? std::string(hdr + 1, hlen - 1) : std::string("seq");
    std::string out;
    size_t at = 0, ri = 0;
    for (const sccg_region& r : regions) {
        out += ">" + name + ":" + std::to_string(r.begin + 1) + "-" + std::to_string(r.end) + (rc_flag ? "/rc\n" : "\n");
        const size_t len = (size_t)(r.end - r.begin);
        if (origin) {   // maximal runs: ascending reference positions, literals, N
            for (int64_t k = seg_off[ri]; k < seg_off[ri + 1]; k++) {
                sccg_segment g;
                memcpy(&g, seq.data + (size_t)k * sizeof g, sizeof g);
                out += std::to_string(g.pos + 1) + "\t" + std::to_string(g.pos + g.len) + "\t";
                if (g.ref >= 0) out += std::to_string(g.ref + 1) + "\t" + std::to_string(g.ref + g.len);
                else out += g.ref == -1 ? "*" : "N";
                out += '\n';
            }
            ri++;
            continue;
        }
        for (size_t k = 0; k < len; k += 50) {
            out.append(seq.data + at + k, len - k < 50 ? len - k : 50);
            out += '\n';
        }
        at += len;
    }
    std::cout << out;
    sccg_buf_free(&seq);
    sccg_reader_close(rd);
    sccg_ctx_destroy(ctx);
    return 0;
}
