// crs.h -- SRS text -> gskyhip_crs (crs.cpp), for host.cpp and ingest.hip.
#pragma once

#include <string>

#include "../../include/gskyhip.h"

namespace gsky {

// "EPSG:n", a PROJ string, WKT1 (a projection family's node, else its
// top-level EPSG authority), "MODIS".  0, or GSKYHIP_E_CRS with *c undefined.
int parse_srs(const char *srs, gskyhip_crs *c);

// The code of the last AUTHORITY["EPSG","n"] node of a WKT (the top-level
// one, as GDAL writes it) into *code; false without such a node.
bool wkt_epsg_code(const std::string &text, int *code);

}  // namespace gsky
