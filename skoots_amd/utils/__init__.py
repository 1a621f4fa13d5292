"""File utilities of the reference's ``skoots/utils``: convert_trch_to_tif, renumber, remove_margin."""
